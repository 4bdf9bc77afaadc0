/*
 * binquant_amd — C ABI of the MI355X (gfx950) technical-indicator engine.
 *
 * This is the drop-in boundary for binquant's indicator hot path. Every entry
 * point takes caller-owned DEVICE buffers (plain pointers + sizes), a
 * hipStream_t (passed as void* so this header needs no HIP include), and
 * returns an int status: 0 = ok, < 0 = error (see BQ_E*). No C++ exception
 * crosses this ABI and the library allocates nothing per call.
 *
 * Data layout (all fp64): structure-of-arrays, one array per OHLCV field,
 * each [S][ld] row-major by symbol (candles of one symbol contiguous), i.e.
 * exactly the memory of S pandas float64 columns laid side by side.
 *
 * Reference interfaces replaced (paths relative to carkod/binquant):
 *   bq_enrich          <- ContextEvaluator.indicators_enrichment
 *                         producers/context_evaluator.py:240-263, i.e. the
 *                         pybinbot.Indicators calls at :249-261
 *                         (moving_averages x3, macd, rsi, bollinguer_spreads,
 *                          set_twap, atr) plus Indicators.mfi
 *                         (strategies/coinrule/price_tracker.py:185) and the
 *                         ema20/ema50 columns of
 *                         market_regime/live_market_context_accumulator.py:266-267
 *   bq_tick            <- per-message recompute of the same columns on the
 *                         latest candle (consumers/klines_provider.py:300-380
 *                         -> context_evaluator.py:347-512), as an O(1) state
 *                         update per symbol
 *   bq_market_features <- LiveMarketContextAccumulator._compute_symbol_features
 *                         market_regime/live_market_context_accumulator.py:244-297
 *                         evaluated at every timestamp of a [S][T] panel
 *   bq_beta_corr       <- ContextEvaluator.dynamic_btc_beta_corr
 *                         producers/context_evaluator.py:154-194
 *   bq_supertrend      <- pybinbot Indicators.set_supertrend
 *                         strategies/coinrule/coinrule.py:143-160
 *   bq_resample*       <- pybinbot Candles.resample(df, "1h")
 *                         producers/context_evaluator.py:403-407
 *   bq_align           <- the benchmark left merge of
 *                         strategies/liquidation_sweep_pump.py:255-263
 *   bq_join_returns,   <- the inner join + rolling beta/corr of
 *   bq_beta_corr_pairs    producers/context_evaluator.py:161-194
 *   bq_store_*         <- MarketStateStore (market_regime/market_state_store.py:14-87)
 *                         and _compute_symbol_features on its histories
 *   bq_parse_kline_events <- json.loads + KlineProduceModel of the websocket
 *                         frames, producers/klines_connector.py:77-164 (host)
 *   bq_micro_regime    <- regime_transitions.py:162-232 (per-symbol micro regime)
 *   bq_symbol_regime_panel <- the same with annotate_context's predecessor rule
 *                         (regime_transitions.py:25-43) at every candle of a panel
 *   bq_context_score   <- context_scoring.py:13-114 + signal_context_scorer.py:15-55
 *   bq_cohort_select   <- the portfolio selectors' winner pick
 *                         (liquidation_sweep_pump.py:38-87, gradual_gainer_retest.py:33-70)
 *   bq_impulse_rider   <- RelativeStrengthImpulseRider._features / _btc_return_at
 *                         (strategies/relative_strength_impulse_rider.py:69-198)
 *   bq_bb_stable       <- LadderDeployer._bb_stable
 *                         (strategies/grid/ladder_deployer.py:42-56)
 *   bq_grid_ladder_replay <- LadderDeployer.signal(): the policy, context and symbol
 *                         gates, _bb_stable, the price and width tests and the
 *                         deployment's range plan (strategies/grid/ladder_deployer.py:58-187)
 *   bq_retest_replay   <- GradualGainerRetest.signal()'s watchlist state machine
 *                         (strategies/gradual_gainer_retest.py:222-308)
 *   bq_spike_fade_replay <- FailedSpikeFade.signal()'s pending-spike state machine
 *                         (strategies/failed_spike_fade.py:596-695)
 *   bq_spike_frames    <- FailedSpikeFade.latest_signal() on every frame of a row, a fresh
 *                         instance per frame (strategies/failed_spike_fade.py:229-594)
 *   bq_spike_frames_capped <- the same on the live store's sliding frame: at most
 *                         frame_cap rows, the first row moving with every candle
 *   bq_price_tracker_replay <- PriceTracker.signal(): the null gate, the oversold test,
 *                         the context score's rejections and the entry cooldown
 *                         (strategies/coinrule/price_tracker.py:83-99, :165-251)
 *   bq_mean_reversion_replay <- MeanReversionFade.signal(): the Wilder RSI hook, the
 *                         rolling means, _resolve_entry, the trend ceiling, the SHORT
 *                         risk profile, the once-per-candle test and the stop-loss cap
 *                         (strategies/mean_reversion_fade.py:88-212, :224-300)
 *   bq_range_fade_replay <- RangeBbRsiMeanReversion.signal(): the frame and null
 *                         gate, regime_routing, _compute_adx, _compute_zscore,
 *                         _resolve_entry's two band rejections and local_score
 *                         (strategies/range_bb_rsi_mean_reversion.py:66-274)
 *   bq_buy_the_dip_replay <- BuyTheDip.signal(): the frame and null gate, the 6 h
 *                         reference candle found by close_time, the change band,
 *                         _allows_entry and the prior-close / EMA20 reclaim
 *                         (strategies/coinrule/buy_the_dip.py:49-85, :127-181)
 *   bq_bb_extreme_replay <- BBExtremeReversion.signal(): the frame and null gate,
 *                         _compute_rsi with pandas' roll_mean over the frame's last
 *                         30 closes, evaluate's band position and the two extremes
 *                         (strategies/coinrule/bb_extreme_reversion.py:134-285)
 *   bq_rs_reversal_replay <- RelativeStrengthReversalRange.signal(): the frame gate,
 *                         regime_routing and the 24 h volume floor, Series.quantile
 *                         over the frame's last 96 volumes
 *                         (strategies/relative_strength_reversal_range.py:56-101)
 *   bq_top_gainer_entry <- TopGainerEarlyMomentum._features / _entry_allows and
 *                         signal()'s two-close confirmation
 *                         (strategies/top_gainer_early_momentum.py:91-253, :363-406)
 *   bq_sweep_select    <- LiquidationSweepPump.signal() between compute_pump_score and
 *                         the selector: the frame gate, _is_candidate, rank_score,
 *                         the routing verdict, and _dispatch_winner's pick per candle
 *                         (strategies/liquidation_sweep_pump.py:271-343, :78-81)
 *   bq_breadth_partial <- the per-symbol sums/counts of
 *                         LiveMarketContextAccumulator._build_context
 *                         market_regime/live_market_context_accumulator.py:135-163
 */
#ifndef BINQUANT_AMD_H
#define BINQUANT_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
#define BQ_OK              0
#define BQ_EINVAL         -1   /* bad argument (null pointer, size, window)   */
#define BQ_EHIP           -2   /* HIP runtime error (launch / memcpy)         */
#define BQ_EALIGN         -3   /* reserved: misaligned buffer                 */
#define BQ_ESTATE         -4   /* state handle misuse                         */

/* ---- canonical enrich column set ---------------------------------------- */
/* Order of the `out` pointer array of bq_enrich / bq_tick. A NULL entry
 * skips that column (its bytes are neither computed nor written). */
enum bq_enrich_col {
  BQ_MA_FAST = 0,     /* "ma_7"        close.rolling(7).mean()              */
  BQ_MA_MID,          /* "ma_25"       close.rolling(25).mean()             */
  BQ_MA_SLOW,         /* "ma_100"      close.rolling(100).mean()            */
  BQ_MACD,            /* "macd"        ema12 - ema26 (adjust=False)         */
  BQ_MACD_SIGNAL,     /* "macd_signal" macd.ewm(span=9, adjust=False)       */
  BQ_RSI,             /* "rsi"         SMA-smoothed RSI(14)                 */
  BQ_BB_UPPER,        /* "bb_upper"    mid + k*std                          */
  BQ_BB_MID,          /* "bb_mid"      close.rolling(20).mean()             */
  BQ_BB_LOWER,        /* "bb_lower"    mid - k*std                          */
  BQ_ATR,             /* "ATR"         true_range.rolling(14).mean()        */
  BQ_TWAP,            /* "twap"        ohlc4.rolling(12).mean()             */
  BQ_EMA_FAST,        /* "ema20"       close.ewm(span=20, adjust=False)     */
  BQ_EMA_SLOW,        /* "ema50"       close.ewm(span=50, adjust=False)     */
  BQ_MFI,             /* "mfi"         money-flow index(14)                 */
  BQ_NUM_ENRICH_COLS
};

/* Input field order of the `in` pointer array. */
enum bq_ohlcv_field { BQ_OPEN = 0, BQ_HIGH, BQ_LOW, BQ_CLOSE, BQ_VOLUME, BQ_NUM_INPUTS };

/* Indicator parameters; defaults (bq_default_params) are the reference's. */
typedef struct bq_params {
  int32_t ma_periods[3];   /* 7, 25, 100   (context_evaluator.py:249-251)   */
  int32_t macd_fast;       /* 12                                            */
  int32_t macd_slow;       /* 26                                            */
  int32_t macd_signal;     /* 9                                             */
  int32_t rsi_window;      /* 14                                            */
  int32_t bb_window;       /* 20                                            */
  int32_t bb_ddof;         /* 1 = pandas default std(); 0 = population      */
  int32_t atr_window;      /* 14           (context_evaluator.py:261)       */
  int32_t twap_window;     /* 12                                            */
  int32_t ema_spans[2];    /* 20, 50       (live_market_context_acc.:266)   */
  int32_t mfi_window;      /* 14           (price_tracker.py:185)           */
  int32_t reserved;
  double  bb_k;            /* 2.0                                           */
} bq_params;

/* Largest rolling window any kernel supports (LDS halo - 2). */
#define BQ_MAX_WINDOW 126

void bq_default_params(bq_params* p);

/* Library / device info. */
const char* bq_version(void);
int bq_device_arch(char* buf, int buflen);   /* e.g. "gfx950" */

/*
 * Full indicator set over a [S][T] panel.
 *   in[BQ_NUM_INPUTS]        device pointers, each [S][ld_in] fp64
 *   out[BQ_NUM_ENRICH_COLS]  device pointers, each [S][ld_out] fp64 (NULL = skip)
 * Warm-up rows are NaN exactly where pandas yields NaN (t < window-1).
 * Input contract: finite candles. The panel is what Candles.pre_process /
 * post_process leave (producers/context_evaluator.py:364-371), which has no
 * NaN rows; a symbol missing candles is a ragged row (enrich_frames), not a
 * NaN row. Missing candles in the live feed go through bq_tick, which keeps
 * pandas' NaN-gap rules.
 */
int bq_enrich(const double* const* in, int64_t S, int64_t T, int64_t ld_in,
              const bq_params* params, double* const* out, int64_t ld_out,
              void* stream);

/* ---- streaming tick path ------------------------------------------------- */
typedef struct bq_state bq_state;   /* opaque, device-resident */

/* Candles in the per-message frame the tick path reproduces: the reference
 * re-fetches KlinesProvider.LIMIT = 400 candles and re-enriches them on every
 * closed kline (consumers/klines_provider.py:40,201-215 ->
 * producers/context_evaluator.py:367-371), so its EMAs are seeded at the
 * frame's first candle. */
#define BQ_TICK_FRAME 400

/* Create state for S symbols. Allocates device memory once (not per tick).
 * bq_state_create = bq_state_create_frame(.., BQ_TICK_FRAME). `frame` = 0
 * keeps unbounded-history EMA carries (the full-series pandas EMA) instead;
 * otherwise BQ_MAX_WINDOW + 2 <= frame <= 2^20 (the frame holds every rolling
 * window, so only the EMA family depends on it). */
int bq_state_create(bq_state** st, int64_t S, const bq_params* params);
int bq_state_create_frame(bq_state** st, int64_t S, const bq_params* params, int64_t frame);
int bq_state_destroy(bq_state* st);
/* Seed the state from a [S][T] history panel (T >= 1): ring of the last
 * BQ_MAX_WINDOW+2 candles, and the last `frame` closes (frame mode) or the
 * exact EMA carries at the last candle (frame 0). */
int bq_state_seed(bq_state* st, const double* const* in, int64_t T, int64_t ld_in,
                  void* stream);
/* Append one candle per symbol. new_ohlcv[BQ_NUM_INPUTS] device pointers of
 * length S; out[BQ_NUM_ENRICH_COLS] device pointers of length S (NULL skip).
 * The outputs are the last row of indicators_enrichment over the symbol's
 * frame (the last `frame` candles; all candles when frame = 0): ema20, ema50,
 * macd and macd_signal bit-equal to pandas' ewm(adjust=False) over that frame.
 * A symbol without a candle this tick passes NaN in all five fields: the
 * outputs are then what pandas gives for a frame with that NaN row — EMAs
 * hold their value and decay their old weight by (1 - alpha)
 * (ewm(adjust=False, ignore_na=False)), windows containing the row are NaN,
 * RSI/MFI count its move as 0 (delta.where(...) fills NaN with 0). */
int bq_tick(bq_state* st, const double* const* new_ohlcv, double* const* out,
            void* stream);
int64_t bq_state_symbols(const bq_state* st);
int64_t bq_state_frame(const bq_state* st);   /* 0 = unbounded */
int64_t bq_state_count(const bq_state* st);   /* candles seen per symbol */

/* ---- market context (breadth / regime) ----------------------------------- */
/* Per-symbol feature columns of _compute_symbol_features, order of `feat`. */
enum bq_feature_col {
  BQ_F_RETURN = 0,    /* return_pct = safe_pct(c_t, c_{t-1})               */
  BQ_F_EMA20,         /* ema over the last `max_bars` closes, span 20       */
  BQ_F_EMA50,         /* span 50                                            */
  BQ_F_TREND,         /* (ema20-ema50)/|ema50|                              */
  BQ_F_ATR_PCT,       /* TR.rolling(14,min_periods=1).mean() / close        */
  BQ_F_BB_WIDTH,      /* 4*std(20,ddof=0)/|mid|                             */
  BQ_NUM_FEATURES
};

/* Breadth partial layout per timestamp: [T][BQ_NUM_PARTIALS] fp64. */
enum bq_partial_col {
  BQ_P_COUNT = 0,     /* symbols with features at t (history >= 2 bars)    */
  BQ_P_ADV,           /* return_pct > 0                                    */
  BQ_P_DEC,           /* return_pct < 0                                    */
  BQ_P_ABOVE20,       /* close > ema20                                     */
  BQ_P_ABOVE50,       /* close > ema50                                     */
  BQ_P_SUM_RET,
  BQ_P_SUM_TREND,
  BQ_P_SUM_ATR_PCT,
  BQ_P_SUM_BB_WIDTH,
  BQ_P_RESERVED,
  BQ_NUM_PARTIALS
};

/*
 * Per-symbol market features at every timestamp, with the accumulator's
 * history cap (MarketStateStore max_bars_per_symbol) applied: the features
 * at t see only candles (t-max_bars, t] (15 <= max_bars <= BQ_MAX_HISTORY).
 * hlc = {high, low, close} device pointers, each [S][ld_in].
 * feat[BQ_NUM_FEATURES] device pointers [S][ld_out] (NULL = skip). Row t = 0
 * (fewer than 2 bars of history -> reference returns None) is NaN.
 * Domain: finite high / low / close (a panel of exchange klines). A candle
 * without a close never reaches the reference's features (MarketStateStore
 * drops it, market_state_store.py:84); histories holding candles without a
 * high / low (which the store keeps) go through bq_store_features, the
 * store path's pandas replay. bq_context_partials has the same domain.
 * Panels with absent candles (NaN close) go through bq_panel_compact +
 * bq_breadth_partial_fresh below.
 */
#define BQ_MAX_HISTORY 512
int bq_market_features(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in,
                       int32_t max_bars, double* const* feat, int64_t ld_out,
                       void* stream);

/*
 * Cross-symbol partial sums per timestamp over the S symbols of this shard,
 * from the feature columns of bq_market_features (all of BQ_F_RETURN,
 * BQ_F_EMA20, BQ_F_EMA50, BQ_F_TREND, BQ_F_ATR_PCT, BQ_F_BB_WIDTH) and close:
 * partial[T][BQ_NUM_PARTIALS] fp64, overwritten. Deterministic (fixed
 * reduction order, no atomics). Feeds an RCCL all-reduce(sum) across shards,
 * then the scalar scoring of _build_context on the host.
 */
int bq_breadth_partial(const double* close, const double* const* feat, int64_t S, int64_t T,
                       int64_t ld_close, int64_t ld_feat, double* partial, void* stream);

/*
 * Fused panel context build (BASELINE configs[4]): the features of
 * bq_market_features reduced straight into the partials of
 * bq_breadth_partial, without writing the feature columns
 * (live_market_context_accumulator.py:95-163 over :244-297 at every t).
 * Replaces bq_market_features + bq_breadth_partial when only the [T][10]
 * partials (and, optionally, the last timestamp's features) are read.
 * hlc = {high, low, close} [S][ld_in]; partial[T][BQ_NUM_PARTIALS]
 * overwritten (column BQ_P_RESERVED = 0). last_feat: NULL, or
 * BQ_NUM_FEATURES device pointers (each NULL or [S]) receiving the features
 * at t = T - 1. workspace: device memory of bq_context_workspace_bytes(S, T)
 * bytes, 256-byte aligned (group records of 4 symbols; the library
 * allocates nothing). Counts equal bq_breadth_partial's; the sums agree to
 * rounding (another fixed order). Deterministic: no atomics.
 */
size_t bq_context_workspace_bytes(int64_t S, int64_t T);
int bq_context_partials(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in,
                        int32_t max_bars, void* workspace, size_t workspace_bytes,
                        double* partial, double* const* last_feat, void* stream);

/*
 * Freshness for panels with late listings, halts, delistings and missing
 * candles. The reference keeps per symbol the candles it received:
 * MarketStateStore drops a candle without a close
 * (market_regime/market_state_store.py:84) and caps the history at the last
 * max_bars of the others (:28); _build_context(ts) admits only the symbols
 * whose last candle is ts (get_fresh_symbols, :49-54), gates on
 * max(40, ceil(0.7 * tracked)) with tracked = every symbol ever seen
 * (live_market_context_accumulator.py:96-102, :196-204), and takes BTC's
 * features from its history as it stands (:105-106).
 *
 * bq_panel_compact: per-row stream compaction. hlc = {high, low, close}
 * [S][ld_in]; candle (s, t) is present iff close[s][t] is finite. Outputs
 * (all overwritten, caller-owned): hlc_out = the present candles of each row
 * packed to the front in order, [S][ld_c], the tail [n_present[s], T) filled
 * with the row's last present candle (1.0 for a row never present) so that
 * bq_market_features runs on it over finite data; rank[S][ld_r] = position k
 * of candle t in the packed row, -1 where absent; n_present[S];
 * first_t[S] = first present t (T if none); n_invalid[S] = candles outside
 * the domain: a +-inf close (treated as absent), or a present candle whose
 * high or low is not finite (packed as it is). Callers reject a panel with
 * n_invalid != 0: such histories belong to the store path (bq_store_features).
 * The features of bq_market_features(hlc_out, max_bars) at [s][k] are then
 * _compute_symbol_features over the store's history of s at the time of its
 * k-th candle. Deterministic; no atomics. T <= 2^31 - 257.
 *
 * bq_breadth_partial_fresh: bq_breadth_partial over the symbols fresh at t.
 * close_c [S][ld_c] and feat_c[BQ_NUM_FEATURES] [S][ld_f] are the packed
 * close and the features computed on the packed panel; for every t the row
 * partial[t] sums, over the symbols with k = rank[s][t] >= 1, the values at
 * [s][k] (columns 0-8, the order of bq_breadth_partial: bit-equal to it when
 * every candle is present). Column BQ_P_RESERVED receives the shard's
 * tracked count at t: the symbols with first_t[s] <= t. rank values must lie
 * in [-1, T); others are skipped. Deterministic; no atomics.
 */
int bq_panel_compact(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in,
                     double* const* hlc_out, int64_t ld_c, int32_t* rank, int64_t ld_r,
                     int32_t* n_present, int32_t* first_t, int32_t* n_invalid, void* stream);
int bq_breadth_partial_fresh(const double* close_c, const double* const* feat_c,
                             const int32_t* rank, const int32_t* first_t, int64_t S, int64_t T,
                             int64_t ld_c, int64_t ld_f, int64_t ld_r, double* partial,
                             void* stream);

/*
 * GradualGainerRetest relative-strength leadership at every prefix t
 * (GradualGainerRetest._leadership_allows + _relative_strengths,
 * strategies/gradual_gainer_retest.py:131-196): open_time [S][ld_ts] int64 ms
 * and close [S][ld_c] of the panel, the benchmark frame bench_ts [nb]
 * (ascending; a duplicated time keeps the later row) / bench_close [nb].
 * Outputs [S][ld_out]: leader (0 / 1 bytes) and rs_2h / rs_6h as the method
 * returns them ((False, 0.0, 0.0) when the strengths are None or the frame
 * is shorter than min_history). One pass: "rs >= sorted(history)[int((n - 1)
 * q)]" is decided by counting the window's entries <= rs (the thresholds are
 * not outputs of the method). Compiled for the strategy's RS_LOOKBACK 96 and
 * long_bars <= 31; other parameters return BQ_EINVAL (the Python layer then
 * runs its staged pipeline). bq_leadership_workspace_bytes returns 0 (the
 * workspace arguments are kept for callers that size one; NULL is fine).
 */
size_t bq_leadership_workspace_bytes(int64_t S, int64_t T);
int bq_leadership(const int64_t* open_time, int64_t ld_ts, const double* close, int64_t ld_c, int64_t S,
                  int64_t T, const int64_t* bench_ts, const double* bench_close, int64_t nb,
                  double rs_quantile, int32_t lookback, int32_t min_history, int32_t min_count,
                  int32_t short_bars, int32_t long_bars, void* workspace, size_t workspace_bytes,
                  uint8_t* leader, double* rs_2h, double* rs_6h, int64_t ld_out, void* stream);

/*
 * GradualGainerRetest.signal()'s watchlist state machine replayed over a panel
 * (strategies/gradual_gainer_retest.py:222-308): column t of row s is what
 * signal() does on the message whose frame is df.iloc[first:t + 1], first =
 * first_t[s] (NULL: 0), after the messages of all earlier candles of the row.
 * Candles t = from_t[s] (NULL: 0) .. lens[s] - 1 (NULL: T) are replayed.
 * open / high / low / close / ema [S][ld_in] (ema: the frame's
 * close.ewm(span=20, adjust=False).mean() column, read at t - 1), open_time
 * [S][ld_ts] int64 ms, leader (bq_leadership's output) and risk_ok (NULL: the
 * risk check always allows) [S][ld_b] 0 / 1 bytes.
 *
 * Per-row state: active, started_at (ms), breakout_level; expires_at is
 * started_at + watch_ms (:119-125). Per candle, in the method's order:
 *   t + 1 - first < min_history       -> SHORT_HISTORY, state untouched (:228-235)
 *   active and open_time > expires_at -> the watch is cleared, D_EXPIRED (:239-241)
 *   idle and leader[t]                -> WATCH_SET: started_at = open_time[t], level =
 *                                        max(high[t-L .. t-1]) skipping NaN (:244-251)
 *   idle                              -> IDLE (:252-253)
 *   a watch in force: support = low[t-1] >= level * sf or low[t-1] >= ema[t-1] * sf,
 *   pullback = close[t-1] >= level * pf, reclaim = close[t] > open[t] and
 *   close[t] > high[t-1] (:255-268); any false -> WATCHING (the failed ones as
 *   D_SUPPORT / D_PULLBACK / D_RECLAIM), all true and risk_ok[t] false ->
 *   RISK_BLOCKED (:271-274), else CANDIDATE and the watch is cleared (:308).
 * Every test is one correctly rounded fp64 multiply and a compare in the
 * method's direction (a NaN fails it): events, details and levels are exact.
 *
 * Domain: open_time strictly ascending within [first, lens) — the
 * strategy_cooldowns check (:275-282) fires only when two messages carry the
 * same open_time and is not built. rank_score, the market-type check and
 * _submit_candidate's message are the caller's.
 *
 * st_active / st_started / st_level [S]: read, then written in place with the
 * state after the row's last replayed candle (a captured graph replays the
 * call as it replays the tick state); all three NULL: start idle, discard.
 * event [S][ld_out] bytes (BQ_RT_*; NO_FRAME where t < from_t or t >= lens),
 * detail [S][ld_out] bytes (NULL = skip), level [S][ld_out] (NULL = skip): the
 * level in force at WATCH_SET / WATCHING / RISK_BLOCKED / CANDIDATE candles,
 * NaN elsewhere. params NULL: the class attributes (bq_retest_default_params).
 * BQ_EINVAL unless 1 <= breakout_lookback <= BQ_RETEST_MAX_LOOKBACK and
 * breakout_lookback < min_history (the level's window stays inside the frame).
 * No workspace, nothing allocated.
 */
#define BQ_RETEST_MAX_LOOKBACK 64
typedef struct bq_retest_params {
  int64_t watch_ms;                         /* WATCHLIST_HOURS * 3_600_000 */
  int32_t min_history, breakout_lookback;   /* MIN_HISTORY 100, BREAKOUT_LOOKBACK 8 */
  double support_factor, pullback_factor;   /* 1 - SUPPORT_TOLERANCE_PCT / 100, 1 - MAX_PULLBACK_PCT, formed by
                                               the caller in fp64 */
} bq_retest_params;
enum { BQ_RT_IDLE = 0, BQ_RT_WATCH_SET, BQ_RT_WATCHING, BQ_RT_RISK_BLOCKED, BQ_RT_CANDIDATE,
       BQ_RT_SHORT_HISTORY, BQ_RT_NO_FRAME = 255 };
enum { BQ_RT_D_SUPPORT = 1, BQ_RT_D_PULLBACK = 2, BQ_RT_D_RECLAIM = 4, BQ_RT_D_EXPIRED = 8 };
void bq_retest_default_params(bq_retest_params* p);
int bq_retest_replay(const double* open, const double* high, const double* low, const double* close,
                     const double* ema, int64_t ld_in, const int64_t* open_time, int64_t ld_ts,
                     const uint8_t* leader, const uint8_t* risk_ok, int64_t ld_b, const int64_t* lens,
                     const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                     const bq_retest_params* params, uint8_t* st_active, int64_t* st_started, double* st_level,
                     uint8_t* event, uint8_t* detail, double* level, int64_t ld_out, void* stream);

/*
 * FailedSpikeFade.signal()'s pending-spike state machine replayed over a panel
 * (strategies/failed_spike_fade.py:596-695): column t of row s is what signal()
 * does on the message whose frame is df.iloc[first:t + 1], first = first_t[s]
 * (NULL: 0), after the messages of all earlier candles of the row. Candles
 * t = max(from_t[s], first) (from_t NULL: 0) .. lens[s] - 1 (NULL: T) are
 * replayed: a candle before first has an empty frame and no message.
 * open / high / close [S][ld_in], open_time [S][ld_ts] int64 ms, source_ok
 * [S][ld_b] 0 / 1 bytes: source_spike_allows (:190-203) of the frame ending at
 * t. src_market / fail_market 0 / 1 bytes with row stride ld_m:
 * source_market_allows / failure_market_allows (:155-188) at t; ld_m == 0: one
 * [T] row shared by all symbols; either pointer NULL: always allowed.
 *
 * Per-row state: active and the pending spike's open_time, high, close (its
 * volume and quote_asset_volume only feed the message text: the source candle
 * is inside the frame, the caller gathers them at t - bars). Per candle, in
 * the method's order (p: the last position in [first, t] whose open_time ==
 * st_open_time; bars = t - p; post_high = max(high[p+1 .. t]), NaN skipped as
 * pandas' max does, a NaN result fails the compare; failed_new_high = high[t]
 * >= st_high and close[t] < open[t] and close[t] < st_close):
 *   # condition                                     event, detail               state     lines
 *   1 t outside [max(from_t, first), lens)          NO_FRAME (255)
 *   2 idle, source_ok[t] and src_market[t]          SOURCE_SET                  st = (open_time[t], high[t],
 *                                                                               close[t]) :618-630
 *   3 idle, otherwise                               IDLE; D_SOURCE and / or     -         :638-646
 *                                                   D_MARKET: the failed side(s)
 *   4 pending, no p found                           CLEARED, D_CANDLE_EXPIRED   cleared   :648-655
 *   5 pending, bars == 0                            SAME_CANDLE                 untouched :660-661
 *   6 pending, bars > window_bars                   CLEARED, D_WINDOW_EXPIRED   cleared   :662-665
 *   7 pending, post_high > st_high * ext_factor     CLEARED, D_EXTENSION        cleared   :667-677
 *   8 pending, not (failed_new_high and             WAITING; D_NEW_HIGH         -         :679-693
 *     fail_market[t])                               (failed_new_high false) and / or D_MARKET
 *   9 pending, failed_new_high and fail_market[t]   CANDIDATE                   cleared   :695
 * Rows 4, 6 and 7 return without looking for a new source on that candle: the
 * candle is consumed (unlike the retest replay's expiry). Every test is a
 * compare in the method's direction (a NaN fails it) and at most one correctly
 * rounded fp64 multiply: events, details, bars and states are exact.
 *
 * Domain: open_time strictly ascending within [first, lens): p is unique.
 * _fiat_order_size, the message text and the dispatch are the caller's.
 *
 * st_active / st_open_time / st_high / st_close [S]: read, then written in
 * place with the state after the row's last replayed candle (0 / NaN where
 * idle; a captured graph carries it); all four NULL: start idle, discard.
 * event [S][ld_out] bytes (BQ_FS_*), detail [S][ld_out] bytes (BQ_FS_D_*, NULL
 * = skip), bars [S][ld_out] bytes (NULL = skip): bars_elapsed at WAITING /
 * CANDIDATE / CLEARED-by-window-or-extension candles (saturated at 255: only a
 * carried-in spike can lie further back), 0 elsewhere. params NULL: the class
 * attributes (bq_spike_fade_default_params). BQ_EINVAL unless 1 <= window_bars
 * <= BQ_SPIKEFADE_MAX_WINDOW, ext_factor is finite, the state pointers are all
 * NULL or all set, and every ld >= T (ld_m: or 0); checked before any launch.
 * S == 0 or T == 0: BQ_OK. No workspace, nothing allocated.
 */
#define BQ_SPIKEFADE_MAX_WINDOW 32
typedef struct bq_spike_fade_params {
  int32_t window_bars;   /* FAILURE_WINDOW_BARS 8 */
  double ext_factor;     /* 1 + MAX_POST_SPIKE_EXTENSION, formed by the caller in fp64 */
} bq_spike_fade_params;
enum { BQ_FS_IDLE = 0, BQ_FS_SOURCE_SET, BQ_FS_WAITING, BQ_FS_CANDIDATE, BQ_FS_CLEARED, BQ_FS_SAME_CANDLE,
       BQ_FS_NO_FRAME = 255 };
enum { BQ_FS_D_SOURCE = 1, BQ_FS_D_MARKET = 2, BQ_FS_D_NEW_HIGH = 4, BQ_FS_D_CANDLE_EXPIRED = 8,
       BQ_FS_D_WINDOW_EXPIRED = 16, BQ_FS_D_EXTENSION = 32 };
void bq_spike_fade_default_params(bq_spike_fade_params* p);
int bq_spike_fade_replay(const double* open, const double* high, const double* close, int64_t ld_in,
                         const int64_t* open_time, int64_t ld_ts, const uint8_t* source_ok, int64_t ld_b,
                         const uint8_t* src_market, const uint8_t* fail_market, int64_t ld_m, const int64_t* lens,
                         const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                         const bq_spike_fade_params* params, uint8_t* st_active, int64_t* st_open_time,
                         double* st_high, double* st_close, uint8_t* event, uint8_t* detail, uint8_t* bars,
                         int64_t ld_out, void* stream);

/*
 * FailedSpikeFade.latest_signal() of every frame of a row
 * (strategies/failed_spike_fade.py:229-594): column t of row s is the method
 * on a FRESH instance (the live behaviour: one strategy instance per message)
 * whose frame is df.iloc[first:t + 1], first = first_t[s] (NULL: 0), with a
 * RangeIndex; candles t = max(from_t[s], first) (NULL: 0) .. lens[s] - 1
 * (NULL: T) are formed. This is the source gate bq_spike_fade_replay's
 * source_ok wants: auto_calibrate's two np.quantile calls (:229-257) and
 * apply_cooldown's walk (:495-520) are frame-wide, so the columns of one
 * whole-row detect() are those of the row's last frame only.
 *
 * in [BQ_NUM_SPIKE_FRAMES_IN] fp64 [S][ld_in]: the columns of detect() that do
 * not depend on the calibrated thresholds, as a frame starting at `first`
 * forms them (the rolling warm-up starts there): volume_ratio,
 * price_change_abs, the forward-filled rolling(60, min_periods=20) quantile of
 * price_change_abs (:376-378, 398), body_size_pct, the rolling
 * (cumulative_price_window) sums of price_change clipped below / above at 0
 * (:408-411), open, close. in_b [BQ_NUM_SPIKE_FRAMES_IN_B] 0 / 1 bytes
 * [S][ld_b]: accel_spike_flag, accel_spike_short_flag (:423-444), upward,
 * downward (:522-531). aligned != 0: column j of an input row holds candle
 * first + j (frame-aligned rows); 0: candle j. Outputs are always indexed by
 * candle.
 *
 * Per frame: theta = (volume_cluster_min_ratio, price_break_base_threshold) =
 * auto_calibrate on rows first .. t (numpy's 'linear' quantile with its
 * two-sided lerp, NaN dropped, +-inf kept: bq_row_quantile's arithmetic, bit
 * for bit; the calibration is skipped, leaving params' two defaults, while
 * either column has no observation), then the flags and labels of row t under
 * theta, and apply_cooldown's verdict on row t among the labels of rows
 * first .. t formed under the same theta (post_spike_cooldown_bars <= 0: label
 * = label_pre). Comparisons only beyond the quantiles: given the inputs, the
 * bytes equal the method's and the thresholds equal numpy's bits.
 *
 * out_b [BQ_NUM_SPIKE_FRAMES_OUT] bytes [S][ld_out] (enum bq_spike_frames_out;
 * NULL table or entry = skip), vcmr / pbbt fp64 [S][ld_out] (NULL = skip):
 * latest_signal()'s fields and the instance's thresholds after the call;
 * 0 / NaN outside the formed candles. workspace: bq_spike_frames_workspace(S,
 * T) bytes of device memory, 8-byte aligned, private to the call until the
 * stream has run it. params NULL: the class attributes
 * (bq_spike_frames_default_params). BQ_EINVAL unless T <=
 * BQ_SPIKE_FRAMES_MAX_T (a frame's sorted prefix lives in LDS), 1 <=
 * volume_cluster_window <= BQ_SPIKE_FRAMES_MAX_WINDOW, 2 <=
 * cumulative_price_window <= BQ_SPIKE_FRAMES_MAX_WINDOW, label_mode in 0..2
 * (last, first, all), post_spike_cooldown_bars < BQ_SPIKE_FRAMES_MAX_COOLDOWN,
 * the quantiles lie in [0, 1], the other parameters are finite and every ld >=
 * T; checked before any launch. S == 0 or T == 0: BQ_OK. Two launches, nothing
 * allocated.
 */
#define BQ_SPIKE_FRAMES_MAX_T 2048
#define BQ_SPIKE_FRAMES_MAX_WINDOW 30
#define BQ_SPIKE_FRAMES_MAX_COOLDOWN 64
typedef struct bq_spike_frames_params {
  int32_t volume_cluster_window, volume_cluster_min_count, cumulative_price_window, label_mode;
  int32_t require_both_patterns, require_bullish_spike, post_spike_cooldown_bars, reserved;
  double cumulative_price_threshold, body_size_pct_min;
  double volume_cluster_min_ratio, price_break_base_threshold;   /* the instance's values before auto_calibrate */
  double volume_quantile, price_base_floor_quantile, min_volume_ratio, min_price_abs_floor;
} bq_spike_frames_params;
enum bq_spike_frames_in {
  BQ_SF_VOLUME_RATIO = 0, BQ_SF_PRICE_CHANGE_ABS, BQ_SF_DYN_THRESHOLD, BQ_SF_BODY_SIZE_PCT, BQ_SF_CUM_POS,
  BQ_SF_CUM_NEG, BQ_SF_OPEN, BQ_SF_CLOSE, BQ_NUM_SPIKE_FRAMES_IN
};
enum bq_spike_frames_in_b {
  BQ_SF_IN_ACCEL = 0, BQ_SF_IN_ACCEL_SHORT, BQ_SF_IN_UPWARD, BQ_SF_IN_DOWNWARD, BQ_NUM_SPIKE_FRAMES_IN_B
};
enum bq_spike_frames_out {
  BQ_SF_LABEL = 0, BQ_SF_LABEL_PRE, BQ_SF_LABEL_SHORT, BQ_SF_LABEL_SHORT_PRE, BQ_SF_VOLUME_CLUSTER_FLAG,
  BQ_SF_PRICE_BREAK_FLAG, BQ_SF_CUM_BREAK_FLAG, BQ_SF_CUM_BREAK_SHORT_FLAG, BQ_SF_ACCEL_FLAG,
  BQ_SF_ACCEL_SHORT_FLAG, BQ_SF_UPWARD, BQ_SF_DOWNWARD, BQ_NUM_SPIKE_FRAMES_OUT
};
void bq_spike_frames_default_params(bq_spike_frames_params* p);
size_t bq_spike_frames_workspace(int64_t S, int64_t T);
int bq_spike_frames(const double* const* in, int64_t ld_in, const uint8_t* const* in_b, int64_t ld_b, int32_t aligned,
                    const int64_t* lens, const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                    const bq_spike_frames_params* params, void* workspace, size_t workspace_bytes, double* vcmr,
                    double* pbbt, uint8_t* const* out_b, int64_t ld_out, void* stream);

/*
 * bq_spike_frames under a SLIDING frame cap: column t of row s is
 * FailedSpikeFade.latest_signal() of a fresh instance whose frame is
 * df.iloc[f:t + 1], f = max(first, t + 1 - frame_cap), with a RangeIndex, and
 * the instance's two calibrated thresholds. This is what the live system
 * sees: the candle provider refetches the last LIMIT candles per message and
 * post_process drops the warm-up rows, so a frame's first row moves with every
 * candle. T is not limited by BQ_SPIKE_FRAMES_MAX_T: a frame's sorted keys (at
 * most frame_cap per column) live in LDS, whatever T.
 *
 * in, in_b, aligned, lens, first_t, from_t, params, the outputs and their
 * conventions are bq_spike_frames': the columns as a frame starting at `first`
 * forms them. in_i [BQ_NUM_SPIKE_FRAMES_IN_I] int32 [S][ld_i], indexed like
 * `in` and holding column indices of `in`: dyn_src, the column of the
 * forward-filled rolling quantile's source (the last column at or before it
 * whose unfilled quantile is not NaN; -1: none), and close_next, the first
 * column at or after it whose close is not NaN (T: none). cap: frame_cap and
 * the three parameters of detect() that only the frame-local columns need.
 *
 * What is frame-local, for a frame [f, t] with f > first; g = close_next[f],
 * the frame's first valid close (rows are candles):
 *   volume_ratio            NaN on rows < f + base_window - 1: no observation
 *                           of the calibration, no bit of the cluster count or
 *                           of vol_cond there
 *   price_change(_abs)      NaN on rows <= g (the pad fill has no source in the
 *                           frame): an observation of the calibration from row
 *                           g + 1 on, price_break_flag False on rows <= g
 *   vol_cond                True on rows < f + cumulative_price_window - 1
 *   the clip sums           NaN on rows < g + cumulative_price_window
 *   the acceleration flags  False on rows <= g and on rows < f + base_window
 *                           - 1 + accel_volume_deriv_window
 *   the rolling(60, min_periods=20) quantile of price_change_abs
 *                           rows >= g + 60: the input's. Rows < g + 60, and
 *                           every later row whose fill's source lies before
 *                           g + 60: roll_quantile of rows g + 1 .. min(row,
 *                           g + 59), NaN below 20 observations
 *   apply_cooldown          walks rows f .. t
 * Every other row of the frame has the input's columns; pandas would form its
 * rolling mean and sums from row f, so they agree to running-sum rounding
 * (the thresholds to ~1e-15 relative, the bytes wherever no comparison is a
 * near-tie). With 1 <= base_window, accel_volume_deriv_window <= 30 and the
 * windows of params a full frame's newest row t = f + frame_cap - 1 >= f + 63
 * lies past every rule above but the quantile's when g > f + 3.
 *
 * workspace: bq_spike_frames_capped_workspace(S, T) bytes, 8-byte aligned.
 * BQ_EINVAL, before any launch: bq_spike_frames' conditions except the one on
 * T; cap NULL, frame_cap outside 64 .. BQ_SPIKE_FRAMES_MAX_T, base_window or
 * accel_volume_deriv_window outside 1 .. BQ_SPIKE_FRAMES_MAX_WINDOW,
 * price_break_dynamic_q outside [0, 1]; in_i NULL or with a NULL entry, ld_i <
 * T; T > 2^30. Two launches, nothing allocated.
 */
#define BQ_SPIKE_FRAMES_MIN_CAP 64
typedef struct bq_spike_frames_cap {
  int32_t frame_cap, base_window, accel_volume_deriv_window, reserved;
  double price_break_dynamic_q;
} bq_spike_frames_cap;
enum bq_spike_frames_in_i { BQ_SF_DYN_SRC = 0, BQ_SF_CLOSE_NEXT, BQ_NUM_SPIKE_FRAMES_IN_I };
size_t bq_spike_frames_capped_workspace(int64_t S, int64_t T);
int bq_spike_frames_capped(const double* const* in, int64_t ld_in, const uint8_t* const* in_b, int64_t ld_b,
                           const int32_t* const* in_i, int64_t ld_i, int32_t aligned, const int64_t* lens,
                           const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                           const bq_spike_frames_params* params, const bq_spike_frames_cap* cap, void* workspace,
                           size_t workspace_bytes, double* vcmr, double* pbbt, uint8_t* const* out_b, int64_t ld_out,
                           void* stream);

/*
 * PriceTracker.signal() replayed over a panel of 5m frames
 * (strategies/coinrule/price_tracker.py:165-324): column t of row s is what
 * signal() does on the message whose frame is df.iloc[first:t + 1], first =
 * first_t[s] (NULL: 0), after the messages of all earlier candles of the row.
 * Candles t = max(from_t[s], first) (from_t NULL: 0) .. lens[s] - 1 (NULL: T)
 * are replayed.
 * close / high / low / volume [S][ld_px], rsi / macd / mfi [S][ld_ind]: the
 * frame's columns; mfi[s][t] is what Indicators.mfi(frame) returns for the
 * frame ending at t (pybinbot's formulas stay outside). high / low / volume are
 * read only by the tail(tail_rows).isnull() test; NULL: the caller knows the
 * column holds no NaN. close_time [S][ld_ct] int64 ms. trend_score [S][ld_tr]
 * or NULL: formed in the pass, (ema_fast - ema_slow) / |ema_slow| (0 where
 * ema_slow == 0) of closes.ewm(span, adjust=False).mean() over the frame, with
 * pandas' update for missing (NaN, +-inf) closes. symbol_rs: the
 * relative_strength_vs_btc of the row's entry in the context snapshot (0.0
 * where it has none, context_scoring.py:26-32), [S] (ld_rs == 0) or [S][ld_rs].
 * ctx [4][ld_ctx]: the rows confidence, long_tailwind, btc_regime_score,
 * market_stress_score of latest_market_context at the candle's message; ctx_T
 * == 1: one context for every candle, ctx_T == T: one per candle. ctx_ok
 * [ctx_T] bytes, 0 where latest_market_context is None (NULL: present). Both
 * are device memory: a captured graph sees values updated in place.
 *
 * Per candle, in the method's order:
 *   # condition                                          status            lines
 *   1 t outside [max(from_t, first), lens)               NO_FRAME
 *   2 t + 1 - first < min_history, or a NaN among the    NOT_READY         :174-181
 *     last tail_rows rows (of the frame) of close, rsi,
 *     macd, high, low, volume (+-inf is not null)
 *   3 not (rsi < rsi_max and macd < macd_max and         NO_SETUP          :194
 *     mfi < mfi_max); a NaN fails
 *   4 ctx_ok == 0                                        NO_CONTEXT        :228
 *   5 followthrough < min_followthrough (D_FOLLOWTHROUGH) CONTEXT_REJECTED :236-242
 *     or risk > max_risk (D_RISK) or confidence <        detail: the bits
 *     min_confidence (D_CONFIDENCE); confidence <= 0
 *     takes _empty_score and so sets D_CONFIDENCE
 *   6 the row has a last entry and                       COOLDOWN          :83-93, :244-250
 *     0 <= close_time[t] - last < cooldown_ms
 *   0 otherwise                                          EMIT              :95-99, :251
 *                                                        last = close_time[t]
 * local_score = 1 + max(0, (rsi_max - rsi) / rsi_max) w_rsi + max(0, (mfi_max
 * - mfi) / mfi_max) w_mfi + min(|macd| macd_scale, 1) w_macd (:198-203); the
 * context score is the LONG branch of RuleBasedMarketContextModel.evaluate
 * with local_features = {"trend_score"} (context_scoring.py:22-85) and
 * SignalContextScorer.adjust_score (signal_context_scorer.py:20-29), each in
 * the reference's operation order: bit for bit the Python floats for a given
 * trend_score. cooldown_ms == 0: strategy_cooldowns is None, the cooldown is
 * never active and nothing is marked. regime_routing, quiet hours, the message
 * text and the dispatch only shape the emitted message: the caller's.
 *
 * st_has / st_last [S]: the row's strategy_cooldowns entry (present, its
 * close_time), read, then written in place (a captured graph carries it); both
 * NULL: start without an entry, discard. status [S][ld_out] bytes (BQ_PT_*),
 * detail [S][ld_out] bytes (NULL = skip), values: NULL or BQ_PT_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_PT_V_* order,
 * NaN where the method did not reach them (status 1-3). params NULL:
 * bq_price_tracker_default_params. BQ_EINVAL, before any launch, unless every
 * ld >= T (ld_rs: or 0), ctx_T is 1 or T, ld_ctx >= ctx_T, the state pointers
 * are both NULL or both set, the thresholds and weights are finite, rsi_max
 * and mfi_max are not 0, min_history >= 1, 1 <= tail_rows <=
 * BQ_PT_MAX_TAIL_ROWS, spans >= 1, cooldown_ms >= 0. S == 0 or T == 0: BQ_OK.
 */
#define BQ_PT_MAX_TAIL_ROWS 64
#define BQ_PT_NVALUES 6
typedef struct bq_price_tracker_params {
  int32_t min_history;        /* 30 (:177) */
  int32_t tail_rows;          /* 5 (:175) */
  int32_t span_fast;          /* 9 (:204) */
  int32_t span_slow;          /* 21 (:205) */
  double rsi_max;             /* 30 */
  double macd_max;            /* 0 */
  double mfi_max;             /* 20 */
  double w_rsi;               /* 0.35 */
  double w_mfi;               /* 0.35 */
  double w_macd;              /* 0.3 */
  double macd_scale;          /* 100 */
  double context_weight;      /* 0.35 (:59-63) */
  double risk_weight;         /* 0.35 */
  double support_weight;      /* 0.2 */
  double min_followthrough;   /* -0.2 (:237) */
  double max_risk;            /* 0.6 (:238) */
  double min_confidence;      /* 0.5 (:239) */
  int64_t cooldown_ms;        /* ENTRY_COOLDOWN_BARS 12 x DEFAULT_INTERVAL_MS 300000; 0: no cooldown */
} bq_price_tracker_params;
enum { BQ_PT_EMIT = 0, BQ_PT_NO_FRAME, BQ_PT_NOT_READY, BQ_PT_NO_SETUP, BQ_PT_NO_CONTEXT, BQ_PT_CONTEXT_REJECTED,
       BQ_PT_COOLDOWN };
enum { BQ_PT_D_FOLLOWTHROUGH = 1, BQ_PT_D_RISK = 2, BQ_PT_D_CONFIDENCE = 4 };
enum { BQ_PT_V_LOCAL = 0, BQ_PT_V_TREND, BQ_PT_V_FOLLOWTHROUGH, BQ_PT_V_RISK, BQ_PT_V_SUPPORT, BQ_PT_V_ADJUSTED };
void bq_price_tracker_default_params(bq_price_tracker_params* p);
int bq_price_tracker_replay(const double* close, const double* high, const double* low, const double* volume,
                            int64_t ld_px, const double* rsi, const double* macd, const double* mfi, int64_t ld_ind,
                            const int64_t* close_time, int64_t ld_ct, const double* trend_score, int64_t ld_tr,
                            const double* symbol_rs, int64_t ld_rs, const double* ctx, int64_t ld_ctx,
                            const uint8_t* ctx_ok, int64_t ctx_T, const int64_t* lens, const int64_t* first_t,
                            const int64_t* from_t, int64_t S, int64_t T, const bq_price_tracker_params* params,
                            uint8_t* st_has, int64_t* st_last, uint8_t* status, uint8_t* detail,
                            double* const* values, int64_t ld_out, void* stream);

/*
 * MeanReversionFade.signal() replayed over a panel of 15m frames
 * (strategies/mean_reversion_fade.py:224-300, with _rsi :88-109, _resolve_entry
 * :111-147, _trend_score :149-155, _stop_loss_pct :163-167, _score :157-161 and
 * the SHORT branch of _risk_profile_allows :170-212): column t of row s is what
 * signal() does on the message whose frame is df_15m.iloc[first:t + 1], first =
 * first_t[s] (NULL: 0), after the messages of all earlier candles of the row.
 * Candles t = max(from_t[s], first) (from_t NULL: 0) .. lens[s] - 1 (NULL: T)
 * are replayed.
 * open / high / low / close / volume [S][ld_px], atr [S][ld_atr] (the enriched
 * frame's ATR column), bb_upper [S][ld_bb] (the bb_high the caller passes; its
 * round_numbers(.., 6) stays with the caller), open_time [S][ld_ot] int64.
 * features: NULL, or BQ_MR_NFEATURES host pointers to [S][ld_ft] doubles in
 * BQ_MR_V_RSI .. BQ_MR_V_TREND order (all set): the method's own rsi,
 * previous_rsi, volume_ma, atr_ma, trend_score, and the pass is point-wise.
 * NULL: they are formed in the pass over the frame starting at first:
 *   rsi          100 g / (g + l), 50.0 where g + l == 0, g / l the ewm(alpha =
 *                1 / rsi_window, min_periods = rsi_window, adjust=False) means
 *                of diff().clip(lower=0) / -diff().clip(upper=0)
 *   previous_rsi rsi of candle t - 1 (NaN at t == first)
 *   trend_score  (ema_fast - ema_slow) / |ema_slow| of ewm(span, adjust=False),
 *                0.0 where ema_slow == 0
 *   volume_ma,   rolling(window).mean() of volume / atr: NaN while the window
 *   atr_ma       reaches before first or holds a missing value
 * with pandas' update for missing (NaN, +-inf) closes. Domain: volume and atr
 * finite or NaN inside the frame (+-inf there is outside the tested domain: the
 * windows treat it as missing, as pandas does).
 * ctx [5][ld_ctx]: the rows market_stress_score, long_regime_score,
 * short_regime_score, btc_regime_score, btc_return of latest_market_context at
 * the candle's message; ctx_T == 1: one context for every candle, ctx_T == T:
 * one per candle. ctx_ok [ctx_T] bytes, 0 where the context is None (NULL:
 * present). The symbol's entry in the context snapshot
 * (resolve_symbol_features): sym_ok bytes (0: None; NULL: no symbol has one, the
 * other four are not read), sym_atr_pct / sym_trend_score doubles, sym_regime /
 * sym_transition bytes (BQ_MR_REGIME_* / BQ_MR_TRANSITION_*, the indices of the
 * micro_regime / micro_regime_transition literals; BQ_MR_NONE for None); each
 * [S] (ld_sym == 0) or [S][ld_sym]. All device memory.
 *
 * Per candle, in the method's order (a NaN fails a comparison as in Python):
 *   #  condition                                               status
 *   1  t outside [max(from_t, first), lens)                    NO_FRAME
 *   2  rsi, previous_rsi, volume_ma, atr, atr_ma or            NOT_READY           :252-257
 *      trend_score not finite (a one-row frame, where the
 *      method itself raises IndexError at :245, is this)
 *   3  atr >= atr_spike_max atr_ma                             ATR_SPIKE           :126
 *   4  volume < volume_ratio_min volume_ma                     LOW_VOLUME          :128
 *   5  high - low <= 0                                         BAD_RANGE           :131-133
 *   6  not (rsi >= rsi_short_min and rsi < previous_rsi and    NO_SETUP            :135-147
 *      close >= bb_upper and close < open and (high -
 *      max(open, close)) / (high - low) >= min_wick_ratio)
 *   7  trend_score > max_trend_score                           TREND_TOO_HIGH      :275
 *   8  ctx_ok == 0                                             NO_CONTEXT          :177
 *   9  market_stress_score >= max_market_stress                STRESS              :179
 *   10 sym_ok and sym_atr_pct > max_symbol_atr_pct             SYMBOL_ATR          :182
 *   11 long_regime_score > short_regime_score + max_gap        LONG_EDGE           :200-204
 *   12 btc_regime_score > 0.15 and btc_return > 0              BTC_UP              :205
 *   13 sym_ok and sym_transition == BREAKOUT_UP                BREAKOUT_UP         :208
 *   14 sym_ok and sym_regime == TREND_UP and                   SYMBOL_TREND_UP     :210
 *      sym_trend_score > 0
 *   15 the row's last emitted candle is open_time[t]           ALREADY_EMITTED     :291
 *   16 stop_loss_pct > max_entry_stop_loss_pct                 STOP_TOO_WIDE       :297
 *   0  otherwise                                               EMIT                :300
 *                                                              last = open_time[t]
 * stop_loss_pct = min(max(atr_stop_mult atr / close 100, 0), 101), 0.0 where
 * close <= 0 (the entry price is the candle's close); score = 1 + max(0, (rsi -
 * rsi_short_min) / (100 - rsi_short_min)); both unrounded: round_numbers(.., 4)
 * and round(.., 4) stay with the caller, as do the FUTURES check, the missing
 * ATR column check, the message and the dispatch. _resolve_entry only ever
 * returns Position.short, so the LONG branch of _risk_profile_allows
 * (:185-198) cannot be reached and is not built.
 *
 * st_has / st_last [S]: the row's strategy_cooldowns entry (present, the open
 * time of the last emitted candle), read, then written in place; both NULL:
 * start without an entry, discard. Domain: open_time strictly ascending within
 * [first, lens). The entry can equal open_time[t] only while it is still the
 * one the call started with (an emit of an earlier candle moves it to a
 * smaller time), so the test is a point-wise compare against the entry state
 * plus "no candle of this call emitted before t", and the state after the call
 * is the open time of the last emitting candle: no serial walk.
 * status [S][ld_out] bytes (BQ_MR_*), values: NULL or BQ_MR_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_MR_V_* order,
 * NaN where the method did not reach them: the five features on every replayed
 * candle, stop_loss_pct on STOP_TOO_WIDE and EMIT, score on EMIT. params NULL:
 * bq_mean_reversion_default_params. BQ_EINVAL, before any launch, unless every
 * ld >= T (ld_sym: or 0), ctx_T is 1 or T, ld_ctx >= ctx_T, the features are
 * all set or the table is NULL, the state pointers are both NULL or both set,
 * the thresholds are finite, rsi_short_min != 100, rsi_window >= 1, the spans
 * >= 1 and 1 <= volume_ma_window, atr_ma_window <= BQ_MR_MAX_WINDOW. S == 0 or
 * T == 0: BQ_OK.
 */
#define BQ_MR_MAX_WINDOW 64
#define BQ_MR_NVALUES 7
#define BQ_MR_NFEATURES 5
#define BQ_MR_NONE 255
#define BQ_MR_REGIME_TREND_UP 0         /* micro_regime "TREND_UP" */
#define BQ_MR_TRANSITION_BREAKOUT_UP 1  /* micro_regime_transition "BREAKOUT_UP" */
typedef struct bq_mean_reversion_params {
  int32_t rsi_window;                /* 14  RSI_WINDOW */
  int32_t volume_ma_window;          /* 20  VOLUME_MA_WINDOW */
  int32_t atr_ma_window;             /* 20  ATR_MA_WINDOW */
  int32_t ema_fast;                  /* 20  EMA_FAST_WINDOW */
  int32_t ema_slow;                  /* 50  EMA_SLOW_WINDOW */
  int32_t reserved;                  /* 0 */
  double rsi_short_min;              /* 76  RSI_SHORT_MIN */
  double volume_ratio_min;           /* 0.8 VOLUME_RATIO_MIN */
  double atr_spike_max;              /* 2.2 ATR_SPIKE_MAX */
  double atr_stop_mult;              /* 2.0 ATR_STOP_MULT */
  double max_entry_stop_loss_pct;    /* 1.5 MAX_ENTRY_STOP_LOSS_PCT */
  double max_trend_score;            /* 0.005 MAX_TREND_SCORE */
  double max_market_stress;          /* 0.25 MAX_MARKET_STRESS_SCORE */
  double max_gap;                    /* 0.02 MAX_CONTEXT_COUNTER_TREND_GAP */
  double max_symbol_atr_pct;         /* 0.03 MAX_SYMBOL_ATR_PCT */
  double min_wick_ratio;             /* 0.0 MIN_REJECTION_WICK_RATIO */
} bq_mean_reversion_params;
enum { BQ_MR_EMIT = 0, BQ_MR_NO_FRAME, BQ_MR_NOT_READY, BQ_MR_ATR_SPIKE, BQ_MR_LOW_VOLUME, BQ_MR_BAD_RANGE,
       BQ_MR_NO_SETUP, BQ_MR_TREND_TOO_HIGH, BQ_MR_NO_CONTEXT, BQ_MR_STRESS, BQ_MR_SYMBOL_ATR, BQ_MR_LONG_EDGE,
       BQ_MR_BTC_UP, BQ_MR_BREAKOUT_UP, BQ_MR_SYMBOL_TREND_UP, BQ_MR_ALREADY_EMITTED, BQ_MR_STOP_TOO_WIDE };
enum { BQ_MR_V_RSI = 0, BQ_MR_V_PREVIOUS_RSI, BQ_MR_V_VOLUME_MA, BQ_MR_V_ATR_MA, BQ_MR_V_TREND, BQ_MR_V_STOP_LOSS,
       BQ_MR_V_SCORE };
void bq_mean_reversion_default_params(bq_mean_reversion_params* p);
int bq_mean_reversion_replay(const double* open, const double* high, const double* low, const double* close,
                             const double* volume, int64_t ld_px, const double* atr, int64_t ld_atr,
                             const double* bb_upper, int64_t ld_bb, const int64_t* open_time, int64_t ld_ot,
                             const double* const* features, int64_t ld_ft, const double* ctx, int64_t ld_ctx,
                             const uint8_t* ctx_ok, int64_t ctx_T, const uint8_t* sym_ok, const double* sym_atr_pct,
                             const double* sym_trend_score, const uint8_t* sym_regime, const uint8_t* sym_transition,
                             int64_t ld_sym, const int64_t* lens, const int64_t* first_t, const int64_t* from_t,
                             int64_t S, int64_t T, const bq_mean_reversion_params* params, uint8_t* st_has,
                             int64_t* st_last, uint8_t* status, double* const* values, int64_t ld_out, void* stream);

/*
 * RangeBbRsiMeanReversion.signal() replayed over a panel of 15m frames
 * (strategies/range_bb_rsi_mean_reversion.py:202-274, with regime_routing
 * :66-98, _compute_adx :101-130, _compute_zscore :132-138, the two rejection
 * tests :140-166 and _resolve_entry :168-196): column t of row s is what
 * signal() does on the message whose frame is df_15m.iloc[first:t + 1], first =
 * first_t[s] (NULL: 0). Candles t = max(from_t[s], first) (from_t NULL: 0) ..
 * lens[s] - 1 (NULL: T) are replayed. The strategy keeps no cooldown entry:
 * there is no state.
 * open / high / low / close / volume [S][ld_px] (volume only feeds the null
 * gate), rsi [S][ld_rsi] (the enriched frame's column), bb_upper / bb_mid /
 * bb_lower [S][ld_bb] (the bb_high / bb_mid / bb_low the caller passes, as the
 * caller rounds them); current_price is the candle's close.
 * features: NULL, or BQ_RF_NFEATURES host pointers to [S][ld_ft] doubles (adx,
 * zscore; both set): the method's own values, and the pass is point-wise. NULL:
 * they are formed in the pass over the frame starting at first:
 *   adx     tr = max(high - low, |high - previous close|, |low - previous
 *           close|) skipping NaN (the frame's first row: high - low), +DM / -DM
 *           0.0 on the first row, the three rolling(adx_window, min_periods =
 *           adx_window) sums, DI = 100 sum / atr_sum, dx = 100 |DI+ - DI-| /
 *           (DI+ + DI-) and 0.0 wherever that is NaN or the total is 0 (the
 *           warm-up included: fillna(0.0)), adx = the rolling(adx_window) mean of
 *           dx, which includes those zeros; 100.0 only while the frame is
 *           shorter than the window. A NaN true range is excluded and counted:
 *           dx is 0.0 while a window holds it.
 *   zscore  (close - mean) / std(ddof=0) over rolling(zscore_window), 0.0 while
 *           the window reaches before first, holds a NaN close, or is one
 *           repeated value (std exactly 0).
 * The sums are direct sums over the window's candles (non-negative terms for
 * the ADX; closes shifted by the candle's own close for the z-score), within
 * 1e-9 relative of pandas' online sums. +-inf in a price is outside this
 * entry's contract.
 * ctx [3][ld_ctx]: the rows regime_is_transitioning (0 / 1),
 * market_stress_score, market_regime (the index of the literal in TREND_UP,
 * TREND_DOWN, RANGE, HIGH_STRESS, TRANSITIONAL; BQ_RF_NONE for None) of
 * latest_market_context at the candle's message; ctx_T == 1: one context for
 * every candle, ctx_T == T: one per candle. ctx_ok [ctx_T] bytes, 0 where the
 * context is None (NULL: present). The symbol's entry in the snapshot
 * (resolve_symbol_features): sym_ok bytes (0: None; NULL: no symbol has one, the
 * other four are not read), sym_regime / sym_transition bytes (indices of the
 * micro_regime / micro_regime_transition literals, BQ_RF_NONE for None),
 * sym_atr_pct / sym_bb_width doubles; each [S] (ld_sym == 0) or [S][ld_sym].
 * All device memory.
 *
 * Per candle, in the method's order (a NaN fails a comparison as in Python):
 *   #  condition                                               status
 *   1  t outside [max(from_t, first), lens)                    NO_FRAME
 *   2  t + 1 - first < min_candles, or a NaN in open / high /  NOT_ENOUGH_DATA     :212
 *      low / close / rsi / volume within the frame's last
 *      min(5, rows) candles
 *   3  ctx_ok == 0                                             NO_CONTEXT          :71
 *   4  regime_is_transitioning != 0                            TRANSITIONING       :73
 *   5  market_stress_score >= max_market_stress                STRESS              :75
 *   6  market_regime == BQ_RF_NONE                             NO_REGIME           :77
 *   7  market_regime != RANGE                                  REGIME_NOT_RANGE    :79
 *   8  sym_ok == 0 (or no snapshot)                            NO_SYMBOL           :81
 *   9  sym_regime != RANGE (None included)                     SYMBOL_NOT_RANGE    :83
 *   10 sym_transition in BREAKOUT_UP, BREAKDOWN,               SYMBOL_TRANSITION   :85
 *      VOLATILITY_EXPANSION
 *   11 sym_atr_pct > max_symbol_atr_pct                        SYMBOL_ATR          :94
 *   12 sym_bb_width > max_symbol_bb_width                      SYMBOL_BB_WIDTH     :96
 *   13 adx > adx_max                                           ADX_TOO_HIGH        :230
 *   14 neither LONG (close <= bb_mid and rsi <= long_rsi_max   NO_SETUP            :168-196
 *      and zscore <= long_zscore_max and the bullish
 *      rejection) nor SHORT (close >= bb_mid and rsi >=
 *      short_rsi_min and zscore >= short_zscore_min and the
 *      bearish rejection); LONG is tested first
 *   0  otherwise                                               EMIT
 * bullish rejection: range = high - low > 0 (NaN passes this test, as in
 * Python), low <= bb_lower (1 + band_touch_tolerance), close > open, (min(open,
 * close) - low) / range >= min_rejection_wick_frac, (close - low) / range >=
 * long_close_position_min. bearish: high >= bb_upper (1 - band_touch_tolerance),
 * close < open, (high - max(open, close)) / range >= min_rejection_wick_frac,
 * (close - low) / range <= short_close_position_max. min / max are Python's.
 * score = 1.0 + min(|zscore| / 3.0, 1.0) 0.35 + max(0.0, (adx_max - adx) /
 * adx_max) 0.25 + r 0.25, r = max(0.0, (long_rsi_max - rsi) / long_rsi_max) for
 * LONG and max(0.0, (rsi - short_rsi_min) / 35.0) for SHORT (the literal 35.0
 * of :271), unrounded and in that operation order. The rounding of the bands,
 * the message text and the dispatch stay with the caller.
 *
 * status [S][ld_out] bytes (BQ_RF_*), values: NULL or BQ_RF_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_RF_V_* order,
 * NaN where the method did not reach them: adx on ADX_TOO_HIGH, NO_SETUP and
 * EMIT, zscore on NO_SETUP and EMIT, direction (bq_direction: 0.0 LONG, 1.0
 * SHORT) and score on EMIT. params NULL: bq_range_fade_default_params.
 * BQ_EINVAL, before any launch, unless every ld >= T (ld_sym: or 0), ctx_T is 1
 * or T, ld_ctx >= ctx_T, the features are both set or the table is NULL, the
 * thresholds are finite, adx_max != 0, long_rsi_max != 0, min_candles >= 1, 1 <=
 * adx_window <= BQ_RF_MAX_ADX_WINDOW and 1 <= zscore_window <=
 * BQ_RF_MAX_ZSCORE_WINDOW (a window and what it carries from the previous
 * 64-candle step fit one step). S == 0 or T == 0: BQ_OK.
 */
#define BQ_RF_MAX_ADX_WINDOW 32
#define BQ_RF_MAX_ZSCORE_WINDOW 64
#define BQ_RF_NVALUES 4
#define BQ_RF_NFEATURES 2
#define BQ_RF_NONE 255
#define BQ_RF_REGIME_RANGE 2                    /* market_regime / micro_regime "RANGE" */
#define BQ_RF_TRANSITION_VOLATILITY_EXPANSION 0 /* micro_regime_transition literals */
#define BQ_RF_TRANSITION_BREAKOUT_UP 1
#define BQ_RF_TRANSITION_BREAKDOWN 2
typedef struct bq_range_fade_params {
  int32_t min_candles;               /* 40  MIN_CANDLES */
  int32_t adx_window;                /* 14  ADX_WINDOW */
  int32_t zscore_window;             /* 20  ZSCORE_WINDOW */
  int32_t reserved;                  /* 0 */
  double adx_max;                    /* 32  ADX_MAX */
  double long_rsi_max;               /* 35  LONG_RSI_MAX */
  double short_rsi_min;              /* 65  SHORT_RSI_MIN */
  double long_zscore_max;            /* -2  LONG_ZSCORE_MAX */
  double short_zscore_min;           /* 2   SHORT_ZSCORE_MIN */
  double band_touch_tolerance;       /* 0.002 BAND_TOUCH_TOLERANCE */
  double max_market_stress;          /* 0.35 MAX_MARKET_STRESS */
  double max_symbol_atr_pct;         /* 0.04 MAX_SYMBOL_ATR_PCT */
  double max_symbol_bb_width;        /* 0.08 MAX_SYMBOL_BB_WIDTH */
  double min_rejection_wick_frac;    /* 0.30 MIN_REJECTION_WICK_FRAC */
  double long_close_position_min;    /* 0.55 LONG_CLOSE_POSITION_MIN */
  double short_close_position_max;   /* 0.45 SHORT_CLOSE_POSITION_MAX */
} bq_range_fade_params;
enum { BQ_RF_EMIT = 0, BQ_RF_NO_FRAME, BQ_RF_NOT_ENOUGH_DATA, BQ_RF_NO_CONTEXT, BQ_RF_TRANSITIONING, BQ_RF_STRESS,
       BQ_RF_NO_REGIME, BQ_RF_REGIME_NOT_RANGE, BQ_RF_NO_SYMBOL, BQ_RF_SYMBOL_NOT_RANGE, BQ_RF_SYMBOL_TRANSITION,
       BQ_RF_SYMBOL_ATR, BQ_RF_SYMBOL_BB_WIDTH, BQ_RF_ADX_TOO_HIGH, BQ_RF_NO_SETUP };
enum { BQ_RF_V_ADX = 0, BQ_RF_V_ZSCORE, BQ_RF_V_DIRECTION, BQ_RF_V_SCORE };
enum { BQ_RF_CTX_TRANSITIONING = 0, BQ_RF_CTX_STRESS, BQ_RF_CTX_REGIME };
void bq_range_fade_default_params(bq_range_fade_params* p);
int bq_range_fade_replay(const double* open, const double* high, const double* low, const double* close,
                         const double* volume, int64_t ld_px, const double* rsi, int64_t ld_rsi,
                         const double* bb_upper, const double* bb_mid, const double* bb_lower, int64_t ld_bb,
                         const double* const* features, int64_t ld_ft, const double* ctx, int64_t ld_ctx,
                         const uint8_t* ctx_ok, int64_t ctx_T, const uint8_t* sym_ok, const uint8_t* sym_regime,
                         const uint8_t* sym_transition, const double* sym_atr_pct, const double* sym_bb_width,
                         int64_t ld_sym, const int64_t* lens, const int64_t* first_t, const int64_t* from_t,
                         int64_t S, int64_t T, const bq_range_fade_params* params, uint8_t* status,
                         double* const* values, int64_t ld_out, void* stream);

/*
 * BuyTheDip.signal() replayed over a panel of 15m frames
 * (strategies/coinrule/buy_the_dip.py:127-243, with _find_reference_price
 * :49-57, _prior_close_and_ema20 :63-71 and _allows_entry :73-85): column t of
 * row s is what signal() does on the message whose frame is df.iloc[first:t +
 * 1], first = first_t[s] (NULL: 0), with current_price = close[t]. The method
 * keeps no state: a column does not depend on the messages before it. Candles
 * t = max(from_t[s], first) (from_t NULL: 0) .. lens[s] - 1 (NULL: T) are
 * replayed.
 * close [S][ld_px]; close_time [S][ld_ct] int64 ms, strictly ascending within
 * [first, lens) (the method's normalize_timestamp is exact on integer ms below
 * 2^53: every time comparison is an integer one). ema20 [S][ld_e] or NULL:
 * formed in the pass, close.ewm(span=ema_span, adjust=False,
 * min_periods=1).mean() over the frame, with pandas' update for missing (NaN,
 * +-inf) closes. market_regime: int8 codes of latest_market_context's
 * market_regime at the candle's message (TREND_UP, TREND_DOWN, RANGE,
 * HIGH_STRESS, TRANSITIONAL; negative: no context, or None), regime_T == 1: one
 * for every candle, regime_T == T: one per candle; NULL: no context.
 * micro_regime: int8 codes of the symbol's micro_regime in that context
 * (TREND_UP, TREND_DOWN, RANGE, VOLATILE, TRANSITIONAL; negative: no features,
 * or None), [S] (ld_m == 0) or [S][ld_m]; NULL: no features. Both are device
 * memory: a captured graph sees values updated in place.
 *
 * Per candle, in the method's order:
 *   # condition                                          status            lines
 *   1 t outside [max(from_t, first), lens)               NO_FRAME
 *   2 t + 1 - first < lookback_candles, or a NaN close   NOT_READY         :137-145
 *     anywhere in the frame (+-inf is a value): once a
 *     row holds one at u >= first, every later candle
 *   3 close_time[t] < start_time_ms                      BEFORE_START      :147-149
 *   4 no u in [first, t] with close_time[u] <=           NO_REFERENCE      :152-156
 *     close_time[t] - lookback_ms
 *   5 change_6h > max_change_pct or                      OUT_OF_BAND       :158-160
 *     change_6h <= min_change_pct (a NaN goes on)
 *   6 market_regime or micro_regime is TREND_UP or       REGIME_BLOCKED    :73-85, :170
 *     TREND_DOWN
 *   7 not (close[t] > close[t - 1] and                   NOT_RECLAIMED     :59-61, :176
 *     close[t] > ema20[t])
 *   0 otherwise                                          EMIT              :183-243
 * reference_price = close[u] of the LARGEST such u (the method scans the frame
 * backwards); change_6h = safe_pct(close[t], reference_price) * 100, safe_pct =
 * (cur - prev) / |prev| and exactly 0.0 where prev == 0 (shared/utils.py:20-23).
 * The autotrade flag and route, quiet hours, the message text and the dispatch
 * only shape the emitted message: the caller's.
 *
 * status [S][ld_out] bytes (BQ_DIP_*), values: NULL or BQ_DIP_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_DIP_V_* order,
 * NaN where the method did not reach them (reference_price / change_6h: status
 * 1-4; ema20: every status but 0 and 7). params NULL:
 * bq_buy_the_dip_default_params. BQ_EINVAL, before any launch, unless every
 * ld >= T (ld_m: or 0), regime_T is 1 or T, the limits are finite with
 * min_change_pct < max_change_pct, lookback_candles >= 2, lookback_ms > 0 and
 * ema_span >= 1. S == 0 or T == 0: BQ_OK.
 */
#define BQ_DIP_NVALUES 3
#define BQ_DIP_REGIME_TREND_UP 0     /* market_regime / micro_regime "TREND_UP" */
#define BQ_DIP_REGIME_TREND_DOWN 1   /* and "TREND_DOWN" */
typedef struct bq_buy_the_dip_params {
  int32_t lookback_candles;   /* 24 LOOKBACK_CANDLES */
  int32_t ema_span;           /* 20 (:67) */
  int64_t lookback_ms;        /* LOOKBACK_HOURS 6 x 3600000 */
  int64_t start_time_ms;      /* START_TIME 2026-04-12 23:21 UTC = 1776036060000 */
  double min_change_pct;      /* -5 (:159) */
  double max_change_pct;      /* -2 (:159) */
} bq_buy_the_dip_params;
enum { BQ_DIP_EMIT = 0, BQ_DIP_NO_FRAME, BQ_DIP_NOT_READY, BQ_DIP_BEFORE_START, BQ_DIP_NO_REFERENCE,
       BQ_DIP_OUT_OF_BAND, BQ_DIP_REGIME_BLOCKED, BQ_DIP_NOT_RECLAIMED };
enum { BQ_DIP_V_REFERENCE = 0, BQ_DIP_V_CHANGE, BQ_DIP_V_EMA };
void bq_buy_the_dip_default_params(bq_buy_the_dip_params* p);
int bq_buy_the_dip_replay(const double* close, int64_t ld_px, const int64_t* close_time, int64_t ld_ct,
                          const double* ema20, int64_t ld_e, const int8_t* market_regime, int64_t regime_T,
                          const int8_t* micro_regime, int64_t ld_m, const int64_t* lens, const int64_t* first_t,
                          const int64_t* from_t, int64_t S, int64_t T, const bq_buy_the_dip_params* params,
                          uint8_t* status, double* const* values, int64_t ld_out, void* stream);

/*
 * BBExtremeReversion.signal() replayed over a panel of 15m frames
 * (strategies/coinrule/bb_extreme_reversion.py:234-285, with evaluate :152-232
 * and _compute_rsi :134-150): column t of row s is what signal() does, were
 * ENABLED true, on the message whose frame is df.iloc[first:t + 1], first =
 * first_t[s] (NULL: 0), with current_price = close[t] and bb_high / bb_mid /
 * bb_low = the bands of candle t. The method keeps no state: a column does not
 * depend on the messages before it. Candles t = max(from_t[s], first) (from_t
 * NULL: 0) .. lens[s] - 1 (NULL: T) are replayed.
 * close [S][ld_px]; bb_upper / bb_mid / bb_lower [S][ld_bb], taken as given: the
 * evaluator's round_numbers(.., 6) on bb_spreads is the caller's step.
 *
 * Per candle, in the method's order:
 *   # condition                                          status            lines
 *   1 t outside [max(from_t, first), lens)               NO_FRAME
 *   2 t + 1 - first < lookback                           NOT_ENOUGH_DATA   :255
 *   3 a NaN among close[t - lookback + 1 .. t]           NULLS             :264
 *     (+-inf is a value)
 *   4 _compute_rsi returned None: rsi_window + 1 >       NO_RSI            :138, :146
 *     lookback, or the last RSI is NaN (a +-inf
 *     difference in the last window, or both means 0)
 *   5 band_span = bb_upper - bb_lower <= 0 (a NaN span   INVALID_BAND      :187
 *     goes on, with band_position 0.5)
 *   6 neither rsi_value <= oversold_rsi and              NO_EXTREME        :194-232
 *     band_position <= max_lower_band_position (buy)
 *     nor rsi_value >= overbought_rsi and band_position
 *     >= min_upper_band_position (sell); buy is tested
 *     first
 *   0 otherwise                                          EMIT
 * The RSI is the frame's own: with g = delta.where(delta > 0, 0.0), q =
 * -delta.where(delta < 0, 0.0) over the differences of df.tail(lookback)'s
 * close (the first is NaN: g 0.0, q -0.0), gain and loss are
 * .rolling(rsi_window).mean() as pandas 2.3.3's roll_mean forms it, replayed
 * from the frame's first row for every candle: an online sum to which a row is
 * added (y = v - ca; t = sum + y; ca = t - sum - y; sum = t) and from which row
 * j - rsi_window is removed first (the same with -v and a compensation of its
 * own); a +-inf row is a missing observation (fewer than rsi_window
 * observations: NaN); the mean is sum / nobs, but the newest value itself where
 * the last nobs rows were all equal, and 0 where no row of the window has the
 * sign bit and the quotient is negative, or every row has it and the quotient
 * is positive. rsi = 100 - 100 / (1 + gain / loss) in IEEE arithmetic (a loss of
 * -0.0 gives 100, 0 / -0.0 gives None), then max(0.0, min(100.0, rsi)).
 * band_position = (close - bb_lower) / band_span where band_span > 0, else 0.5;
 * bb_width = band_span / bb_mid and distance_from_mid_pct = (close - bb_mid) /
 * bb_mid * 100 where bb_mid > 0, else 0.0 (a NaN bb_mid: 0.0). ENABLED, the
 * autotrade flag and route, the message text and the dispatch are the caller's.
 *
 * status [S][ld_out] bytes (BQ_BBX_*), values: NULL or BQ_BBX_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_BBX_V_* order,
 * NaN where the method did not reach evaluate (status 1-3): rsi_value (50.0 on
 * NO_RSI), band_position, bb_width, distance_from_mid_pct, and direction
 * (bq_direction: 0.0 LONG for a buy, 1.0 SHORT for a sell) on EMIT alone.
 * params NULL: bq_bb_extreme_default_params. BQ_EINVAL, before any launch, unless
 * every ld >= T, the four thresholds are finite, 1 <= lookback <=
 * BQ_BBX_MAX_LOOKBACK (a candle's frame reaches at most one 64-candle step back)
 * and rsi_window >= 1. S == 0 or T == 0: BQ_OK.
 */
#define BQ_BBX_MAX_LOOKBACK 64
#define BQ_BBX_NVALUES 5
typedef struct bq_bb_extreme_params {
  int32_t lookback;                 /* 30  LOOKBACK_CANDLES */
  int32_t rsi_window;               /* 2   DEFAULT_RSI_WINDOW */
  double oversold_rsi;              /* 5   DEFAULT_OVERSOLD_RSI */
  double overbought_rsi;            /* 95  DEFAULT_OVERBOUGHT_RSI */
  double max_lower_band_position;   /* 0   DEFAULT_MAX_LOWER_BAND_POSITION */
  double min_upper_band_position;   /* 1   DEFAULT_MIN_UPPER_BAND_POSITION */
} bq_bb_extreme_params;
enum { BQ_BBX_EMIT = 0, BQ_BBX_NO_FRAME, BQ_BBX_NOT_ENOUGH_DATA, BQ_BBX_NULLS, BQ_BBX_NO_RSI, BQ_BBX_INVALID_BAND,
       BQ_BBX_NO_EXTREME };
enum { BQ_BBX_V_RSI = 0, BQ_BBX_V_POSITION, BQ_BBX_V_WIDTH, BQ_BBX_V_DISTANCE, BQ_BBX_V_DIRECTION };
void bq_bb_extreme_default_params(bq_bb_extreme_params* p);
int bq_bb_extreme_replay(const double* close, int64_t ld_px, const double* bb_upper, const double* bb_mid,
                         const double* bb_lower, int64_t ld_bb, const int64_t* lens, const int64_t* first_t,
                         const int64_t* from_t, int64_t S, int64_t T, const bq_bb_extreme_params* params,
                         uint8_t* status, double* const* values, int64_t ld_out, void* stream);

/*
 * RelativeStrengthReversalRange.signal() replayed over a panel of 15m frames
 * (strategies/relative_strength_reversal_range.py:75-101, with regime_routing
 * :56-73): column t of row s is what signal() does on the message whose frame
 * is df.iloc[first:t + 1], first = first_t[s] (NULL: 0). The method keeps no
 * state: a column does not depend on the messages before it. Candles t =
 * max(from_t[s], first) (from_t NULL: 0) .. lens[s] - 1 (NULL: T) are replayed.
 * volume [S][ld_v]. The context of candle t's message: context_ok (NULL: a
 * context is present), market_regime (int8, an index into "TREND_UP",
 * "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL"; negative: None) and
 * average_return, each of length ctx_T, 1 (one context for every candle) or T.
 * The symbol's entry in the context's snapshot: features_ok (NULL: present;
 * false: the context has no features for the symbol) and
 * relative_strength_vs_btc, [S] with ld_sym 0, or [S][ld_sym] per candle.
 *
 * Per candle, in the method's order (the first match wins):
 *   # condition                                          status            lines
 *   1 t outside [max(from_t, first), lens)               NO_FRAME
 *   2 t + 1 - first < window                             SHORT_FRAME       :85
 *   3 context_ok false                                   NO_CONTEXT        :61
 *   4 market_regime < 0                                  REGIME_NONE       :63
 *   5 market_regime != RANGE                             NOT_RANGE         :65
 *   6 average_return >= avg_return_max (a NaN goes on)   MARKET_NOT_WEAK   :67
 *   7 features_ok false                                  NO_FEATURES       :69
 *   8 relative_strength_vs_btc <= rs_min (a NaN goes on) RS_INSUFFICIENT   :71
 *   9 volume[t] <= volume_floor (a NaN on either side    DEAD_TAPE         :100
 *     goes on)
 *   0 otherwise                                          EMIT
 * volume_floor = df["volume"].tail(window).quantile(quantile), which is
 * Series.quantile, np.percentile(method="linear") over the non-NaN rows, not
 * pandas' rolling quantile: +-inf is a value; with s the n non-NaN values of
 * volume[t - window + 1 .. t] ascending (n == 0: NaN), vi = (n - 1) * quantile
 * (the quantile after pandas' and numpy's round trip, (quantile * 100) / 100),
 * fl = floor(vi), g = vi - fl, a = s[fl], b = s[min(fl + 1, n - 1)], d = b - a,
 * the floor is b - d * (1 - g) where g >= 0.5 and a + d * g otherwise, without
 * FMA and also where g == 0: a finite a beside an infinite b gives NaN, and
 * the message goes out. The floor of a zero is +0.0 or -0.0. The message
 * always carries autotrade = False and the route "range_rs_reversal"; its
 * text, quote_asset_volume and the dispatch are the caller's.
 *
 * status [S][ld_out] bytes (BQ_RSR_*), values: NULL or BQ_RSR_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_RSR_V_* order:
 * volume_floor, NaN for status 1-8. params NULL: bq_rs_reversal_default_params.
 * BQ_EINVAL, before any launch, unless every ld >= T (ld_sym: or 0), ctx_T is 1
 * or T, 1 <= window <= BQ_RSR_MAX_WINDOW (window + 63 <= 256 sorted slots),
 * 0 <= quantile <= 1 and the two thresholds are finite. S == 0 or T == 0: BQ_OK.
 */
#define BQ_RSR_MAX_WINDOW 192
#define BQ_RSR_NVALUES 1
#define BQ_RSR_REGIME_RANGE 2   /* market_regime "RANGE" */
typedef struct bq_rs_reversal_params {
  int32_t window;          /* 96    VOLUME_WINDOW */
  int32_t reserved;
  double quantile;         /* 0.20  VOLUME_PERCENTILE */
  double avg_return_max;   /* -0.02 AVG_RETURN_MAX */
  double rs_min;           /* 0.05  RS_VS_BTC_MIN */
} bq_rs_reversal_params;
enum { BQ_RSR_EMIT = 0, BQ_RSR_NO_FRAME, BQ_RSR_SHORT_FRAME, BQ_RSR_NO_CONTEXT, BQ_RSR_REGIME_NONE, BQ_RSR_NOT_RANGE,
       BQ_RSR_MARKET_NOT_WEAK, BQ_RSR_NO_FEATURES, BQ_RSR_RS_INSUFFICIENT, BQ_RSR_DEAD_TAPE };
enum { BQ_RSR_V_FLOOR = 0 };
void bq_rs_reversal_default_params(bq_rs_reversal_params* p);
int bq_rs_reversal_replay(const double* volume, int64_t ld_v, const uint8_t* context_ok, const int8_t* market_regime,
                          const double* average_return, int64_t ctx_T, const uint8_t* features_ok,
                          const double* relative_strength_vs_btc, int64_t ld_sym, const int64_t* lens,
                          const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                          const bq_rs_reversal_params* params, uint8_t* status, double* const* values,
                          int64_t ld_out, void* stream);

/*
 * RelativeStrengthImpulseRider._features at every prefix t
 * (strategies/relative_strength_impulse_rider.py:92-198, with _btc_return_at,
 * :69-90): column t of row s is the method on df.iloc[first:t + 1], first =
 * first_t[s] (NULL: 0; the rows Candles.post_process dropped), against the
 * benchmark frame bench_ts [nb] (ascending; a duplicated time resolves to
 * its last row, as the method's backwards scan does) / bench_close [nb]
 * (both may be NULL when nb == 0). open / high / low / close [S][ld_in], atr
 * (the frame's ATR column) [S][ld_atr], open_time [S][ld_ts] int64 ms.
 * Trigger = candle t - 1, confirmation = candle t; the benchmark return's
 * anchor is four POSITIONS before the matched row (:85).
 *
 * status [S][ld_out] bytes: the first failing check in the method's order
 * (BQ_IR_*, 0 = relative_strength_impulse_confirmed); BQ_IR_NO_FRAME where
 * t >= lens[s] (lens NULL: T). values: BQ_IR_NVALUES device pointers
 * [S][ld_out] in the order below (a NULL entry, or values == NULL, skips the
 * column), each the method's own expression (bit-exact) where status is 0
 * and NaN elsewhere (the method returns None there). params NULL: the class
 * attributes (bq_impulse_default_params). BQ_EINVAL for min_history < 7 (the
 * stencil reaches t - 6). No workspace, nothing allocated.
 */
#define BQ_IMPULSE_TILE 1024   /* candles per workgroup tile of both kernels */
#define BQ_IR_CONFIRMED              0   /* :197 */
#define BQ_IR_SHORT_HISTORY          1   /* history_too_short (:99) */
#define BQ_IR_INVALID_VALUES         2   /* invalid_candle_values (:124) */
#define BQ_IR_INVALID_ANCHORS        3   /* invalid_return_anchors (:130) */
#define BQ_IR_BTC_UNAVAILABLE        4   /* btc_return_unavailable (:137) */
#define BQ_IR_RANGE_INVALID          5   /* confirmation_range_invalid (:144) */
#define BQ_IR_NOT_READY              6   /* indicators_not_ready (:159) */
#define BQ_IR_IMPULSE_RANGE          7   /* impulse_outside_range (:161) */
#define BQ_IR_DID_NOT_CROSS          8   /* impulse_did_not_cross_threshold (:165) */
#define BQ_IR_BTC_TOO_HIGH           9   /* btc_return_too_high (:167) */
#define BQ_IR_RS_TOO_LOW            10   /* relative_strength_too_low (:169) */
#define BQ_IR_ATR_TOO_HIGH          11   /* atr_pct_too_high (:171) */
#define BQ_IR_DID_NOT_HOLD          12   /* confirmation_did_not_hold_trigger_close (:173) */
#define BQ_IR_CONFIRMATION_NEGATIVE 13   /* confirmation_return_negative (:175) */
#define BQ_IR_CLOSE_NOT_NEAR_HIGH   14   /* confirmation_close_not_near_high (:177) */
#define BQ_IR_NO_FRAME             255   /* t >= lens[s]: no such prefix frame */
/* value columns: impulse_return_1h, previous_impulse_return_1h, btc_return_1h,
 * relative_strength_1h, trigger_return_15m, confirmation_return_15m,
 * confirmation_close_location, atr_pct, entry_limit_price (:187-195) */
#define BQ_IR_NVALUES 9
typedef struct bq_impulse_params {
  double min_impulse;          /* MIN_IMPULSE_RETURN_1H 0.05 */
  double max_impulse;          /* MAX_IMPULSE_RETURN_1H 0.18 */
  double min_rs;               /* MIN_RELATIVE_STRENGTH_1H 0.08 */
  double max_btc_return;       /* MAX_BTC_RETURN_1H 0.01 */
  double min_conf_return;      /* MIN_CONFIRMATION_RETURN 0.0 */
  double min_close_location;   /* MIN_CONFIRMATION_CLOSE_LOCATION 0.70 */
  double max_atr_pct;          /* MAX_ATR_PCT 0.06 */
  double entry_factor;         /* 1 - RETEST_DISCOUNT_PCT / 100, formed by the caller in fp64 */
  int32_t min_history;         /* MIN_HISTORY 20 (>= 7) */
  int32_t reserved;
} bq_impulse_params;
void bq_impulse_default_params(bq_impulse_params* p);
int bq_impulse_rider(const double* open, const double* high, const double* low, const double* close,
                     int64_t ld_in, const double* atr, int64_t ld_atr, const int64_t* open_time,
                     int64_t ld_ts, const int64_t* lens, const int64_t* first_t, int64_t S, int64_t T,
                     const int64_t* bench_ts, const double* bench_close, int64_t nb,
                     const bq_impulse_params* params, uint8_t* status, double* const* values,
                     int64_t ld_out, void* stream);

/*
 * LadderDeployer._bb_stable(n, max_change_pct) at every prefix t
 * (strategies/grid/ladder_deployer.py:42-56) on df.iloc[first:t + 1]:
 * bb_upper / bb_mid / bb_lower [S][ld_in], 1 <= n <= BQ_BB_STABLE_MAX_N
 * (the strategy: 8, 20.0). stable [S][ld_out] (0 / 1 bytes): at least n rows,
 * each of the last n with bb_mid > 0 and width = (upper - lower) / mid > 0
 * (a NaN row passes both tests, as in Python), and
 * abs((w[t] - w[t-n+1]) / w[t-n+1]) * 100 <= max_change_pct. change_pct
 * [S][ld_out] (NULL = skip): that expression (bit-exact) where the method
 * reaches it, NaN where it returns earlier. Columns t >= lens[s]: 0 / NaN.
 */
#define BQ_BB_STABLE_MAX_N 64
int bq_bb_stable(const double* bb_upper, const double* bb_mid, const double* bb_lower, int64_t ld_in,
                 const int64_t* lens, const int64_t* first_t, int64_t S, int64_t T, int32_t n,
                 double max_change_pct, uint8_t* stable, double* change_pct, int64_t ld_out, void* stream);

/*
 * LadderDeployer.signal(current_price, bb_high, bb_mid, bb_low) replayed over
 * a [S][T] panel of 15m frames (strategies/grid/ladder_deployer.py:58-187):
 * column t of row s is the method on the message whose frame is
 * df_15m.iloc[first:t + 1], first = first_t[s] (NULL: 0); candles
 * max(from_t[s], first) .. lens[s] - 1 are replayed (NULL: 0 / T). ENABLED and
 * the market_type != FUTURES return (:61-67) are the caller's; the method
 * keeps no state. One launch, nothing allocated, nothing read back.
 *
 * close [S][ld_c] is current_price. bb_upper / bb_mid / bb_lower [S][ld_bb]
 * are the frame's columns, which _bb_stable iterates over. bb_high /
 * bb_mid_arg / bb_low [S][ld_bands] are the bands as passed to signal() (the
 * evaluator rounds them); all three NULL, or equal to the frame's pointers
 * and pitch: the frame's columns are what signal() receives, and each is read
 * once. Per candle time, each of length ctx_T, 1 (one message) or T:
 * policy_ok (grid_only_policy.allow_grid_ladder; NULL: allowed), ctx_ok (0:
 * latest_market_context is None; NULL: present), market_regime (int8, an
 * index into "TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL";
 * negative: None) and long_regime_score. The symbol's entry in the snapshot,
 * [S] with ld_sym 0 or [S][ld_sym] per candle: sym_ok (0:
 * resolve_symbol_features gave None; NULL: no symbol has features),
 * sym_micro_regime / sym_micro_transition (indices into the micro_regime /
 * micro_regime_transition literals, BQ_MR_NONE for None), sym_above_ema20 /
 * sym_above_ema50, sym_rs_vs_btc and sym_atr_pct.
 *
 * Per candle, in the method's order (the first match wins):
 *    # condition                                              status             lines
 *    1 t outside [max(from_t, first), lens)                   NO_FRAME
 *    2 policy_ok false                                        POLICY             :70-75
 *    3 ctx_ok false                                           NO_CONTEXT         :76
 *    4 market_regime != RANGE                                 NOT_RANGE          :79
 *    5 sym_ok false, or micro_regime != RANGE                 MICRO_REGIME       :83-88
 *    6 micro_transition is BREAKDOWN, VOLATILITY_EXPANSION    SYMBOL_TRANSITION  :89
 *      or ENTERED_TREND_DOWN
 *    7 neither above_ema20 nor above_ema50                    BELOW_EMAS         :92
 *    8 rs_vs_btc <= 0 (a NaN goes on)                         RS_NOT_POSITIVE    :95
 *    9 long_regime_score < min_long_score (a NaN goes on)     LONG_SCORE_LOW     :98
 *   10 not _bb_stable(n, max_change_pct) (bq_bb_stable's      BB_EXPANDING       :101-106
 *      rules, on the frame's columns)
 *   11 not (bb_low < close < bb_high) (false on any NaN)      PRICE_OUTSIDE      :109
 *   12 not (min_width_pct <= range_width_pct <=               RANGE_WIDTH        :115-119
 *      max_width_pct)
 *    0 otherwise                                              EMIT
 * range_width_pct = ((bb_high - bb_low) / bb_mid_arg) * 100 if bb_mid_arg > 0
 * else 0 (a NaN or non-positive mid: 0). On EMIT, raw = (atr_pct * 100) *
 * atr_multiplier, breakout_buffer_pct = max(min_buffer_pct, min(max_buffer_pct,
 * raw)) with Python's min / max (the first argument unless the second compares
 * strictly beyond it: a NaN atr_pct gives max_buffer_pct), breakout_low =
 * bb_low * (1 - buffer / 100), breakout_high = bb_high * (1 + buffer / 100);
 * range_low / range_high are bb_low / bb_high themselves. Every value is the
 * method's IEEE operations in its order (bit-exact).
 *
 * status [S][ld_out] bytes (BQ_GL_*), values: NULL or BQ_GL_NVALUES host
 * pointers to [S][ld_out] doubles (a NULL entry is skipped) in BQ_GL_V_* order:
 * bb_change_pct where the method reached _bb_stable and its walk reached :55,
 * range_width_pct on RANGE_WIDTH and EMIT, breakout_buffer_pct / breakout_low /
 * breakout_high on EMIT; NaN elsewhere. params NULL:
 * bq_grid_ladder_default_params. BQ_EINVAL, before any launch, unless every
 * ld >= T (ld_sym: or 0), ctx_T is 1 or T, 1 <= n <= BQ_BB_STABLE_MAX_N, the
 * thresholds are finite and S * ceil(T / BQ_GRID_LADDER_TILE) fits a grid.
 * S == 0 or T == 0: BQ_OK.
 */
#define BQ_GRID_LADDER_TILE 1024   /* candles per workgroup tile */
#define BQ_GL_NVALUES 5
#define BQ_GL_REGIME_RANGE 2                    /* market_regime / micro_regime "RANGE" */
#define BQ_GL_TRANSITION_VOLATILITY_EXPANSION 0 /* micro_regime_transition literals */
#define BQ_GL_TRANSITION_BREAKDOWN 2
#define BQ_GL_TRANSITION_ENTERED_TREND_DOWN 6
typedef struct bq_grid_ladder_params {
  int32_t n;               /* 8    MIN_BB_WIDTH_STABILITY_CANDLES */
  int32_t reserved;
  double max_change_pct;   /* 20.0 MAX_BB_WIDTH_CHANGE_PCT */
  double min_width_pct;    /* 1.5  MIN_RANGE_WIDTH_PCT */
  double max_width_pct;    /* 8.0  MAX_RANGE_WIDTH_PCT */
  double min_buffer_pct;   /* 0.5  MIN_BREAKOUT_BUFFER_PCT */
  double max_buffer_pct;   /* 4.0  MAX_BREAKOUT_BUFFER_PCT */
  double atr_multiplier;   /* 1.5  BREAKOUT_ATR_MULTIPLIER */
  double min_long_score;   /* 0.2  MIN_LONG_REGIME_SCORE */
} bq_grid_ladder_params;
enum { BQ_GL_EMIT = 0, BQ_GL_NO_FRAME, BQ_GL_POLICY, BQ_GL_NO_CONTEXT, BQ_GL_NOT_RANGE, BQ_GL_MICRO_REGIME,
       BQ_GL_SYMBOL_TRANSITION, BQ_GL_BELOW_EMAS, BQ_GL_RS_NOT_POSITIVE, BQ_GL_LONG_SCORE_LOW, BQ_GL_BB_EXPANDING,
       BQ_GL_PRICE_OUTSIDE, BQ_GL_RANGE_WIDTH };
/* value columns: bb_change_pct, range_width_pct, breakout_buffer_pct, breakout_low, breakout_high */
enum { BQ_GL_V_BB_CHANGE = 0, BQ_GL_V_RANGE_WIDTH, BQ_GL_V_BUFFER, BQ_GL_V_BREAKOUT_LOW, BQ_GL_V_BREAKOUT_HIGH };
void bq_grid_ladder_default_params(bq_grid_ladder_params* p);
int bq_grid_ladder_replay(const double* close, int64_t ld_c, const double* bb_upper, const double* bb_mid,
                          const double* bb_lower, int64_t ld_bb, const double* bb_high, const double* bb_mid_arg,
                          const double* bb_low, int64_t ld_bands, const uint8_t* policy_ok, const uint8_t* ctx_ok,
                          const int8_t* market_regime, const double* long_regime_score, int64_t ctx_T,
                          const uint8_t* sym_ok, const uint8_t* sym_micro_regime,
                          const uint8_t* sym_micro_transition, const uint8_t* sym_above_ema20,
                          const uint8_t* sym_above_ema50, const double* sym_rs_vs_btc, const double* sym_atr_pct,
                          int64_t ld_sym, const int64_t* lens, const int64_t* first_t, const int64_t* from_t,
                          int64_t S, int64_t T, const bq_grid_ladder_params* params, uint8_t* status,
                          double* const* values, int64_t ld_out, void* stream);

/*
 * TopGainerEarlyMomentum at every candle of the panel, one pass over the row
 * (strategies/top_gainer_early_momentum.py): the features of the prefix frame
 * (_features, :91-159), the breakout gate (_entry_allows, :161-188) and
 * signal()'s two-close confirmation (:190-202, :363-406). Column t of row s
 * stands for the frame df.iloc[first:t + 1], first = first_t[s] (NULL: 0),
 * t < lens[s] (NULL: T). open / high / low / close / volume [S][ld_in];
 * quote_volume [S][ld_qv] (NULL: the reference's fall-backs volume * close
 * and volume_ma * close, :110-119); atr [S][ld_atr], the frame's ATR column
 * (NULL: 0.0, :120); risk_ok [S][ld_risk] bytes, _risk_profile_allows per
 * candle (:204-234; NULL: allowed).
 *
 * Features: previous_high = the NaN-skipping max of the lookback_high highs
 * before t (:108); volume_ma / quote_volume_ma = rolling(volume_window).mean()
 * with pandas' rules (min_periods = window, +-inf missing, the same-value
 * rule; :109, :115-117); the returns over 4 / 8 / 24 candles (:141-143); the
 * extension anchor close[first + max(0, t - first - full_extension_bars)]
 * with its window and scaled cap (:124-132); ema20 / ema50 =
 * close.ewm(span, adjust=False).mean() seeded at first (:153-154; a missing
 * close decays the old weight as pandas does). The point-wise values are the
 * reference's own expressions, bit for bit; the two ewm columns and the two
 * volume ratios agree with pandas to rounding.
 *
 * entry [S][ld_out] bytes: the feature status (history_too_short :93,
 * invalid_candle_values :105 — Python's min(): a NaN first argument sticks, a
 * NaN elsewhere is skipped —, indicators_not_ready :157), else the first
 * failing check of _entry_allows, else 0 (top_gainer_breakout_ignition).
 * status [S][ld_out] bytes: signal()'s outcome for the message whose newest
 * candle is t: history_too_short (t + 1 - first < min_history + 2, :364), else
 * entry[t - 2] if non-zero (:369-377), else the two confirmation rules on
 * close[t - 1] / close[t] (:198-201), else RISK_REJECTED where risk_ok[t] is
 * 0 (:397-406), else 0 (top_gainer_breakout_two_close_confirmation). Both are
 * BQ_TGE_NO_FRAME where t >= lens[s].
 *
 * values: BQ_TGE_NVALUES device pointers [S][ld_out] in _features' key order
 * (:133-156; a NULL entry, or values == NULL, skips the column): the prefix
 * frame's value where the feature status is ready, NaN elsewhere. score /
 * stop_loss_pct [S][ld_out] (NULL = skip): _score of the breakout candle
 * t - 2 (:246-253) and _stop_loss_pct(close[t], atr[t]) (:236-243, Python's
 * min / max argument order for a NaN) where status is 0 or RISK_REJECTED, NaN
 * elsewhere. Both are UNROUNDED: the reference rounds them with pybinbot's
 * round_numbers(.., 4), which is not part of it; rounding is the host's step.
 *
 * Not built: _already_emitted (:255-258, :410-413) compares candle open times
 * for equality only, so it cannot fire between distinct candles of a panel;
 * it stays with the host, as do the market-type check and the message.
 *
 * params NULL: the class attributes (bq_top_gainer_default_params). BQ_EINVAL
 * for a NULL required pointer (the five inputs, status, entry), a pitch < T,
 * lookback_high / volume_window / full_extension_bars outside
 * 1..BQ_TGE_MAX_LOOKBACK (the ring's halo), min_history < 25 (the returns
 * reach t - 24), S or T beyond 2^31. S == 0 or T == 0: BQ_OK, no launch. No
 * workspace, nothing allocated.
 */
#define BQ_TGE_MAX_LOOKBACK 96
#define BQ_TGE_CONFIRMED          0   /* entry: top_gainer_breakout_ignition (:188); status: ..._two_close_confirmation (:202) */
#define BQ_TGE_SHORT_HISTORY      1   /* history_too_short (:94, :365) */
#define BQ_TGE_INVALID_CANDLE     2   /* invalid_candle_values (:106) */
#define BQ_TGE_NOT_READY          3   /* indicators_not_ready (:158) */
#define BQ_TGE_NOT_BREAKING       4   /* not_breaking_recent_high (:164) */
#define BQ_TGE_NOT_ABOVE_EMAS     5   /* not_above_ema20_and_ema50 (:166) */
#define BQ_TGE_NOT_GREEN          6   /* candle_not_green_enough (:168) */
#define BQ_TGE_CANDLE_EXTENDED    7   /* single_candle_too_extended (:170) */
#define BQ_TGE_HOUR_EXTENDED      8   /* one_hour_move_too_extended (:172) */
#define BQ_TGE_EXTENSION          9   /* extension_move_too_extended (:174) */
#define BQ_TGE_NOT_ACCELERATING  10   /* momentum_not_accelerating (:179) */
#define BQ_TGE_SIX_HOUR          11   /* six_hour_move_not_confirmed (:181) */
#define BQ_TGE_VOLUME_LOW        12   /* volume_ratio_too_low (:183) */
#define BQ_TGE_NOT_NEAR_HIGH     13   /* close_not_near_high (:185) */
#define BQ_TGE_UPPER_WICK        14   /* upper_wick_too_large (:187) */
#define BQ_TGE_FIRST_CONFIRM     15   /* first_confirmation_did_not_hold_breakout (:199) */
#define BQ_TGE_SECOND_CONFIRM    16   /* second_confirmation_did_not_clear_breakout_close (:201) */
#define BQ_TGE_RISK_REJECTED     17   /* _risk_profile_allows refused (:397-406) */
#define BQ_TGE_NO_FRAME         255   /* t >= lens[s]: no such message */
/* value columns, _features' key order (:133-156): close, open, high, low,
 * volume, quote_volume, previous_high, return_1h, return_2h, return_6h,
 * extension_return, extension_window_bars, extension_cap, candle_return,
 * volume_ratio, quote_volume_ratio, range_position, upper_wick_fraction,
 * ema20, ema50, atr */
#define BQ_TGE_NVALUES 21
typedef struct bq_top_gainer_params {
  int32_t lookback_high;          /* LOOKBACK_HIGH_WINDOW 48 */
  int32_t volume_window;          /* VOLUME_WINDOW 32 */
  int32_t min_history;            /* MIN_HISTORY 56 (>= 25) */
  int32_t full_extension_bars;    /* FULL_EXTENSION_WINDOW_BARS 96 */
  double min_candle_return;       /* MIN_CANDLE_RETURN 0.01 */
  double max_candle_return;       /* MAX_CANDLE_RETURN 0.10 */
  double min_return_1h;           /* MIN_RETURN_1H 0.05 */
  double min_return_2h;           /* MIN_RETURN_2H 0.08 */
  double min_return_6h;           /* MIN_RETURN_6H 0.07 */
  double max_return_1h;           /* MAX_RETURN_1H 0.20 */
  double max_extension;           /* MAX_EXTENSION_RETURN 0.50 */
  double min_short_extension_cap; /* MIN_SHORT_HISTORY_EXTENSION_CAP 0.25 */
  double min_volume_ratio;        /* MIN_VOLUME_RATIO 1.75 */
  double min_range_position;      /* MIN_CLOSE_RANGE_POSITION 0.75 */
  double max_upper_wick;          /* MAX_UPPER_WICK_FRACTION 0.30 */
  double atr_stop_mult;           /* ATR_STOP_MULT 2.2 (:64) */
  double min_stop_loss_pct;       /* MIN_STOP_LOSS_PCT 1.5 (:65) */
  double max_stop_loss_pct;       /* MAX_STOP_LOSS_PCT 2.0 (:66) */
} bq_top_gainer_params;
void bq_top_gainer_default_params(bq_top_gainer_params* p);
int bq_top_gainer_entry(const double* open, const double* high, const double* low, const double* close,
                        const double* volume, int64_t ld_in, const double* quote_volume, int64_t ld_qv,
                        const double* atr, int64_t ld_atr, const uint8_t* risk_ok, int64_t ld_risk,
                        const int64_t* lens, const int64_t* first_t, int64_t S, int64_t T,
                        const bq_top_gainer_params* params, uint8_t* status, uint8_t* entry, double* score,
                        double* stop_loss_pct, double* const* values, int64_t ld_out, void* stream);

/*
 * LiquidationSweepPump's candidate gate and the cohort winner at every candle
 * of the panel (strategies/liquidation_sweep_pump.py): what signal() does
 * between compute_pump_score and the portfolio selector (:302-343), and the
 * pick LiquidationSweepPortfolioSelector._dispatch_winner makes among a candle
 * time's candidates (:78-81).
 *
 * cols: BQ_SW_NCOLS device pointers (a host table), each [S][ld_in] fp64, the
 * values _is_candidate reads in its order (:272-286): pump_score,
 * score_threshold, momentum_atr, close, prior_high, close_location,
 * relative_volume, volume_threshold, trend_score, ema20, relative_strength,
 * btc_momentum_3, btc_trend_score. score_cross [S][ld_b] bytes. route_ok
 * [S][ld_r] bytes, long_entry_routing's verdict per cell (:338-343; NULL:
 * allowed). lens / first_t [S] (NULL: T / 0). symbol_rank [S]: the position of
 * the row's symbol in the str order of the names (NULL: the row index).
 *
 * Column u is the TRIGGER candle: the decision signal() takes on df.iloc[-2]
 * at the message whose frame is df.iloc[first : u + 2] (the newest candle
 * u + 1 is the message). Domain: the rows share one open-time grid, so column
 * u of every row is one candle time — one cohort of the selector (the cohort
 * stage assumes the same); the columns are the caller's, computed on frames
 * that start at `first` (the panel convention of the pump features). Only
 * columns of [t_lo, t_hi) are read or written.
 *
 * status [S][ld_out] bytes: the first failing check in the method's order
 * (BQ_SW_*): NO_FRAME where u + 1 >= lens[s] or u < first; SHORT_FRAME where
 * u + 2 - first < min_frame (:314); NOT_FINITE (:287); the score cross and
 * the nine compares of :290-299, each in the method's direction;
 * THRESHOLD_NONPOSITIVE (:331); ROUTE_REFUSED (:343); else 0, a candidate the
 * method would submit. rank_score [S][ld_out] fp64 (NULL = skip): pump_score /
 * score_threshold, one correctly rounded divide (:333), where status is 0; NaN
 * elsewhere.
 *
 * winner / winner_score [T] (winner_score NULL = skip): per column the row of
 * the candidate with the largest (rank_score, symbol_rank) — max(key=
 * (rank_score, symbol)) of :78-81 — and its rank_score; -1 / NaN for a column
 * without a candidate. Equal ranks are a caller error (two rows, one symbol);
 * then the larger row wins. A rank_score that overflowed to +inf beats every
 * finite one. The result does not depend on the launch geometry.
 *
 * workspace: bq_sweep_select_workspace(S, T) bytes of device memory, 8-byte
 * aligned, the caller's; no initialisation needed, nothing is allocated.
 * Ranges of fewer than 64 columns (the cohort's one column) run a lane per
 * row, wider ones (the panel replay) a lane per candle.
 *
 * params NULL: the class attributes (bq_sweep_default_params). BQ_EINVAL,
 * before any launch: cols or an entry of it NULL; score_cross, status, winner
 * or workspace NULL (or workspace misaligned); ld_in, ld_b or ld_out < T, ld_r
 * < T with route_ok given; t_lo < 0, t_hi > T, t_lo > t_hi; a non-finite
 * threshold or min_momentum_atr > max_momentum_atr; S or T above 0x7fffffff
 * (or a range whose workgroup count is). S == 0, T == 0 or t_lo == t_hi:
 * BQ_OK, no launch.
 */
#define BQ_SW_NCOLS 13
#define BQ_SW_CANDIDATE               0   /* submitted to the selector (:438) */
#define BQ_SW_SHORT_FRAME             1   /* len(df) < SCORE_LOOKBACK + COMPRESSION_BARS + 2 (:314) */
#define BQ_SW_NOT_FINITE              2   /* a required value is not finite (:287) */
#define BQ_SW_NO_CROSS                3   /* score_cross (:290) */
#define BQ_SW_MOMENTUM_ATR            4   /* MIN <= momentum_atr <= MAX (:291) */
#define BQ_SW_NOT_ABOVE_PRIOR_HIGH    5   /* close > prior_high (:292) */
#define BQ_SW_CLOSE_LOCATION          6   /* close_location >= MIN_CLOSE_LOCATION (:293) */
#define BQ_SW_VOLUME                  7   /* relative_volume >= volume_threshold (:294) */
#define BQ_SW_TREND                   8   /* trend_score > 0 (:295) */
#define BQ_SW_BELOW_EMA20             9   /* close > ema20 (:296) */
#define BQ_SW_RELATIVE_STRENGTH      10   /* relative_strength > 0 (:297) */
#define BQ_SW_BTC_MOMENTUM           11   /* btc_momentum_3 > 0 (:298) */
#define BQ_SW_BTC_TREND              12   /* btc_trend_score > 0 (:299) */
#define BQ_SW_THRESHOLD_NONPOSITIVE  13   /* score_threshold <= 0 (:331) */
#define BQ_SW_ROUTE_REFUSED          14   /* long_entry_routing refused (:343) */
#define BQ_SW_NO_FRAME              255   /* u + 1 >= lens[s] or u < first: no such message */
typedef struct bq_sweep_params {
  double min_momentum_atr;     /* MIN_MOMENTUM_ATR 0.75 */
  double max_momentum_atr;     /* MAX_MOMENTUM_ATR 3.0 */
  double min_close_location;   /* MIN_CLOSE_LOCATION 0.70 */
  int32_t min_frame;           /* SCORE_LOOKBACK + COMPRESSION_BARS + 2 = 56 (:314) */
  int32_t reserved;
} bq_sweep_params;
void bq_sweep_default_params(bq_sweep_params* p);
int64_t bq_sweep_select_workspace(int64_t S, int64_t T);
int bq_sweep_select(const double* const* cols, int64_t ld_in, const uint8_t* score_cross, int64_t ld_b,
                    const uint8_t* route_ok, int64_t ld_r, const int64_t* lens, const int64_t* first_t,
                    const int32_t* symbol_rank, int64_t S, int64_t T, int64_t t_lo, int64_t t_hi,
                    const bq_sweep_params* params, uint8_t* status, double* rank_score, int64_t ld_out,
                    int64_t* winner, double* winner_score, void* workspace, void* stream);

/* ---- benchmark-relative statistics ---------------------------------------- */
/*
 * Rolling beta and correlation of log returns vs the benchmark
 * (ContextEvaluator.dynamic_btc_beta_corr, producers/context_evaluator.py:154-194)
 * at every timestamp: close [S][ld_in], btc_close [T] (index-aligned with the
 * panel), window 2..BQ_MAX_WINDOW (reference: 50). beta/corr [S][ld_out]
 * (NULL = skip). NaN where t < window, beta NaN where var(btc) == 0. Inputs
 * must be finite and positive (the reference dropna()s only the first return).
 */
int bq_beta_corr(const double* close, const double* btc_close, int64_t S, int64_t T, int64_t ld_in,
                 int32_t window, double* beta, double* corr, int64_t ld_out, void* stream);

/* ---- rolling-window statistics (strategy feature pipelines) ---------------- */
#define BQ_MAX_ROLLING_WINDOW 96
enum bq_roll_mode {
  BQ_ROLL_QUANTILE = 0, BQ_ROLL_MEDIAN = 1, BQ_ROLL_MEAN = 2, BQ_ROLL_SUM = 3,
  BQ_ROLL_VAR = 4,   /* ddof 1 */
  BQ_ROLL_STD = 5,   /* ddof 1 */
  BQ_ROLL_VAR0 = 6,  /* ddof 0 */
  BQ_ROLL_STD0 = 7,  /* ddof 0 */
  BQ_ROLL_EWM = 8,   /* bq_rolling_batch only: ewm(alpha, adjust=False, min_periods) */
  BQ_ROLL_FFILL = 9, /* bq_rolling_batch only: ffill() (leading NaNs stay), shift 0;
                        Series.pct_change's default fill_method='pad' */
  BQ_ROLL_ISUM = 10, /* rolling sum of a series whose values are integers with
                        |sum| < 2^53 (counts of boolean flags): pandas' result
                        is then exact in any summation order, so the window is
                        summed directly (no sequential replay); same values,
                        same-value rule and min_periods as BQ_ROLL_SUM */
  BQ_ROLL_QLOWER = 11 /* quantile(q, interpolation="lower"): the int((n-1) q)-th
                        smallest of the window's n values, no interpolation —
                        sorted(history)[int((len(history) - 1) * q)] of
                        GradualGainerRetest._leadership_allows
                        (strategies/gradual_gainer_retest.py:182-187) */
};
/*
 * out = x.shift(shift).rolling(window, min_periods).<mode>() per symbol row,
 * pandas semantics (NaNs skipped, NaN below min_periods; quantile = linear
 * interpolation, q in [0, 1]; q = 0 / 1 give rolling min / max; sum / mean
 * compensated, pandas' same-value rule for mean / sum / var / std; an empty
 * window sums to 0 when min_periods is 0). Replaces the
 * pandas rolling calls of strategies/activity_burst_pump.py:58-63,134-152,
 * strategies/liquidation_sweep_pump.py:218-245, strategies/failed_spike_fade.py:376-378.
 * x, out [S][ld] fp64 device pointers; window <= BQ_MAX_ROLLING_WINDOW;
 * ld_out <= BQ_MAX_ROLL_LD (else BQ_EINVAL).
 */
#define BQ_MAX_ROLL_LD 4194303   /* 64 rows x ld_out x 8 B < 2^31 (32-bit buffer offsets) */
int bq_rolling(const double* x, int64_t S, int64_t T, int64_t ld_in, int32_t window, int32_t min_periods,
               int32_t shift, int32_t mode, double q, double* out, int64_t ld_out, void* stream);

/*
 * out = x.shift(shift).rolling(window, min_periods).quantile(q) as bq_rolling
 * (BQ_ROLL_QUANTILE), and cross[t] = (x[t] >= out[t]) & (x[t-1] < out[t-1])
 * as one byte per candle (pandas comparisons: NaN compares false; 0 at t = 0)
 * — LiquidationSweepPump's score_threshold and score_cross
 * (strategies/liquidation_sweep_pump.py:231-239) in one pass where the
 * sliding-window kernel runs (else the quantile, then a flag pass). cross:
 * uint8 [S][ld_cross] device pointer.
 */
int bq_rolling_quantile_cross(const double* x, int64_t S, int64_t T, int64_t ld_in, int32_t window,
                              int32_t min_periods, int32_t shift, double q, double* out, int64_t ld_out,
                              uint8_t* cross, int64_t ld_cross, void* stream);

/*
 * Many independent rolling / ewm series over one [S][T] shape in one call
 * (the strategy pipelines issue 5-18 of them per frame batch, e.g.
 * strategies/failed_spike_fade.py:260-357): one launch per kernel family
 * instead of one per series, so lane-per-symbol replays of different series
 * run side by side. Jobs are read from HOST memory (copied into the launch).
 */
#define BQ_MAX_ROLL_JOBS 16
typedef struct bq_roll_job {
  const double* x;         /* [S][ld_in] device pointer                        */
  double* out;             /* [S][ld_out] device pointer                       */
  int64_t ld_in, ld_out;
  int32_t window, min_periods, shift, mode;   /* mode: bq_roll_mode            */
  double q;                /* quantile                                         */
  double alpha;            /* BQ_ROLL_EWM                                      */
  int64_t rows;            /* rows of this job's x / out, 1 <= rows <= S (a    */
                           /* benchmark series beside the panel); 0 = all S.  */
                           /* Moments / ewm / ffill only: order statistics    */
                           /* need 0 or S.                                     */
  int32_t panel;           /* 1: sum / mean (window + shift <= 128) and ewm    */
                           /* time-parallel, within rounding of pandas (1e-9) */
                           /* instead of the bit-exact sequential replay      */
  int32_t reserved;
} bq_roll_job;
int bq_rolling_batch(const bq_roll_job* jobs, int32_t n_jobs, int64_t S, int64_t T, void* stream);
/*
 * bq_rolling_batch with crossing flags: for a BQ_ROLL_QUANTILE job i with
 * cross[i] != NULL (uint8 [S][ld_cross[i]] device pointer; the job on all S
 * rows), also cross[i][t] = (x[t] >= out[t]) & (x[t-1] < out[t-1]) as
 * bq_rolling_quantile_cross — formed in the sliding-window kernel's steps
 * where that kernel runs the job. cross / ld_cross: host arrays of n_jobs
 * (cross NULL: none).
 */
int bq_rolling_batch_cross(const bq_roll_job* jobs, int32_t n_jobs, int64_t S, int64_t T, uint8_t* const* cross,
                           const int64_t* ld_cross, void* stream);

/*
 * out = x.ewm(alpha=alpha, adjust=False, min_periods=min_periods).mean()
 * (ignore_na=False: NaN gaps decay the old weight) per symbol row, the exact
 * pandas recursion. Replaces strategies/liquidation_sweep_pump.py:215-217,
 * :265-266 and strategies/mean_reversion_fade.py:94-99.
 */
int bq_ewm(const double* x, int64_t S, int64_t T, int64_t ld_in, double alpha, int32_t min_periods, double* out,
           int64_t ld_out, void* stream);

/*
 * LiquidationSweepPump's per-symbol ewm columns in panel mode (time-parallel,
 * within rounding of pandas; strategies/liquidation_sweep_pump.py:206-217,
 * :252-253): atr = TR.ewm(alpha=1/14, adjust=False, min_periods=14).mean() of
 * the true range of (high, low, close) — formed in the kernel, no TR column —
 * and ema20 / ema50 = close.ewm(span=20 / 50, adjust=False).mean(), in one
 * pass per row; trend_score (NULL = skip) = (ema20 - ema50) / ema50 (:254).
 * Inputs [S][ld_in], outputs [S][ld_out] fp64. Feeds bq_pump_features.
 */
int bq_pump_ewm(const double* high, const double* low, const double* close, int64_t S, int64_t T, int64_t ld_in,
                double* atr, double* ema20, double* ema50, double* trend_score, int64_t ld_out, void* stream);

/* ---- whole-series order statistics and label cooldown ---------------------- */
/*
 * out[s] = numpy.quantile(x[s][~isnan], q) (numpy 'linear' method, numpy's
 * two-sided lerp), NaN for a row without observations. Replaces the
 * np.quantile calls of FailedSpikeFade.auto_calibrate
 * (strategies/failed_spike_fade.py:229-257). One number per row, for the
 * row's newest candle alone: the volume floor of
 * RelativeStrengthReversalRange.signal() at every candle, behind its route
 * gate, is bq_rs_reversal_replay's (the same index and lerp). out: S doubles.
 */
int bq_row_quantile(const double* x, int64_t S, int64_t T, int64_t ld_in, double q, double* out, void* stream);

/*
 * FailedSpikeFade.apply_cooldown (strategies/failed_spike_fade.py:495-520):
 * a label (nonzero byte) within `bars` candles of the last kept label is
 * cleared in kept[] and set in suppressed[]. label/kept/suppressed: uint8
 * [S][ld] device pointers.
 */
int bq_cooldown(const uint8_t* label, int64_t S, int64_t T, int64_t ld_in, int32_t bars, uint8_t* kept,
                uint8_t* suppressed, int64_t ld_out, void* stream);

/* ---- fused strategy stages -------------------------------------------------- */
/*
 * LiquidationSweepPump.compute_pump_score (strategies/liquidation_sweep_pump.py:
 * 195-269) in one pass per row, panel mode: every column but the two rolling
 * quantiles (score_threshold / volume_threshold) and score_cross, with the
 * volume.shift(1).rolling(volume_lookback).mean() and the
 * high / low .shift(1).rolling(compression_bars).max() / .min() windows and
 * close.pct_change(momentum_bars) (pad-filled) formed in the kernel.
 * in = {high, low, close, volume, candidate_atr, ema20, ema50} [S][ld_in]
 * fp64 (the three ewm columns from bq_pump_ewm; ema20 / ema50 may both be
 * NULL when out[BQ_PUMP_EMA20 / EMA50 / TREND_SCORE] are NULL); bench = {ffilled
 * benchmark close, its ewm(span=20), ewm(span=50)} [T] fp64 (the benchmark
 * left-merged on the panel's open_time grid); out[BQ_NUM_PUMP_COLS] [S][ld_out]
 * fp64 (NULL = skip). momentum_bars <= 31, volume_lookback and
 * compression_bars <= 30.
 */
enum bq_pump_col {
  BQ_PUMP_CANDIDATE_ATR = 0, BQ_PUMP_MOMENTUM_3, BQ_PUMP_RELATIVE_VOLUME, BQ_PUMP_COMPRESSION, BQ_PUMP_SCORE,
  BQ_PUMP_PRIOR_HIGH, BQ_PUMP_CLOSE_LOCATION, BQ_PUMP_EMA20, BQ_PUMP_EMA50, BQ_PUMP_TREND_SCORE,
  BQ_PUMP_MOMENTUM_ATR, BQ_PUMP_BTC_MOMENTUM_3, BQ_PUMP_BTC_TREND_SCORE, BQ_PUMP_RELATIVE_STRENGTH,
  BQ_NUM_PUMP_COLS
};
int bq_pump_features(const double* const* in, int64_t S, int64_t T, int64_t ld_in, const double* const* bench,
                     int32_t momentum_bars, int32_t volume_lookback, int32_t compression_bars, double* const* out,
                     int64_t ld_out, void* stream);
/*
 * The same pass with the three per-symbol ewm columns formed inside it
 * (candidate_atr = TR.ewm(alpha=1/14, adjust=False, min_periods=14).mean(),
 * ema20 / ema50 = close.ewm(span=20 / 50, adjust=False).mean(),
 * liquidation_sweep_pump.py:206-217, 252-253; within rounding of pandas, a
 * row with a missing / infinite value continuing with pandas' recursion):
 * in = {high, low, close, volume} only; out[BQ_PUMP_CANDIDATE_ATR /
 * BQ_PUMP_EMA20 / BQ_PUMP_EMA50] must be non-NULL.
 */
int bq_pump_features_ewm(const double* const* in, int64_t S, int64_t T, int64_t ld_in, const double* const* bench,
                         int32_t momentum_bars, int32_t volume_lookback, int32_t compression_bars,
                         double* const* out, int64_t ld_out, void* stream);

/*
 * ActivityBurstPump.compute_indicators (strategies/activity_burst_pump.py:51-158)
 * around the score's rolling quantile, bit for bit with the staged pipeline:
 * bq_burst_features forms every column of :58-133 from in = {open, high, low,
 * close, volume, quote_volume, baseline_volume, baseline_quote_volume}
 * [S][ld_in] fp64 (the two baselines: volume.shift(2).rolling(19).median(),
 * bq_rolling_batch; quote_volume and its baseline NULL without a quote
 * volume column: the reference's neutral fallbacks), out_f[BQ_NUM_BURST_F]
 * fp64 and out_b[BQ_NUM_BURST_B] uint8 [S][ld_out] (NULL = skip), all_flags
 * uint8 [S][ld_out]: the AND of the six flags (NULL = skip). bq_burst_qualify:
 * qualified_signal from the score, its threshold (rolling quantile) and
 * all_flags (:140-156), cooldown_bars <= 8; ld_b = the byte arrays' stride.
 */
typedef struct bq_burst_params {
  double volume_multiplier, quote_volume_multiplier, price_threshold, min_baseline_volume;
  double min_range_frac, min_body_frac, max_close_to_high;
  int32_t min_recent_up_closes;   /* the effective minimum (1 without a quote volume) */
  int32_t reserved;
} bq_burst_params;
enum bq_burst_fcol {
  BQ_BURST_BASELINE_VOLUME_SAFE = 0, BQ_BURST_VOLUME_RATIO, BQ_BURST_BASELINE_QUOTE_VOLUME_SAFE,
  BQ_BURST_QUOTE_VOLUME_RATIO, BQ_BURST_PRICE_JUMP, BQ_BURST_RANGE_FRAC, BQ_BURST_BODY_FRAC, BQ_BURST_CLOSE_TO_HIGH,
  BQ_BURST_RECENT_UP_CLOSES, BQ_BURST_SCORE, BQ_NUM_BURST_F
};
enum bq_burst_bcol {
  BQ_BURST_IS_BULLISH = 0, BQ_BURST_VOL_SPIKE, BQ_BURST_QUOTE_VOL_SPIKE, BQ_BURST_PRICE_JUMP_FLAG,
  BQ_BURST_RANGE_EXPANSION_FLAG, BQ_BURST_BODY_QUALITY_FLAG, BQ_BURST_TREND_QUALITY_FLAG, BQ_NUM_BURST_B
};
int bq_burst_features(const double* const* in, int64_t S, int64_t T, int64_t ld_in, const bq_burst_params* p,
                      double* const* out_f, uint8_t* const* out_b, uint8_t* all_flags, int64_t ld_out, void* stream);
int bq_burst_qualify(const double* score, const double* threshold, const uint8_t* all_flags, int64_t S, int64_t T,
                     int64_t ld_in, int64_t ld_b, int32_t cooldown_bars, uint8_t* qualified, void* stream);

/*
 * FailedSpikeFade.detect (strategies/failed_spike_fade.py:260-544) in two
 * passes per row around auto_calibrate. bq_spike_base: in = {open, high, low,
 * close, volume, quote_volume, ffilled close, price_std (close, base window),
 * volume_std (base window), close std 8, close std 20, body_size_pct std 10}
 * [S][ld_in] fp64 (the std columns: bq_rolling_batch's bit-exact replays) ->
 * compute_base_features' and the early features' columns (out_f
 * [BQ_NUM_SPIKE_BASE_F] fp64, out_b [BQ_NUM_SPIKE_BASE_B] uint8, NULL = skip),
 * the rolling means / sums (min_periods = window) formed in the kernel;
 * base_window, streak_length <= 30. bq_spike_flags: in = {open, close, ffilled
 * close, volume_ratio, |pct change| rolling quantile} [S][ld_in], vcmr / pbbt
 * [S] (the calibrated volume-cluster ratio and price-break base) -> the flag
 * columns and preliminary labels of :360-488 (cooldown: bq_cooldown).
 */
typedef struct bq_spike_params {
  int32_t volume_cluster_window, volume_cluster_min_count, cumulative_price_window, accel_volume_deriv_window;
  int32_t label_mode;   /* 0 last, 1 first, 2 all */
  int32_t require_both_patterns, require_bullish_spike, reserved;
  double cumulative_price_threshold, accel_volume_deriv_min, accel_price_change_min, body_size_pct_min;
} bq_spike_params;
enum bq_spike_base_fcol {
  BQ_SPIKE_PRICE_CHANGE = 0, BQ_SPIKE_PRICE_CHANGE_ABS, BQ_SPIKE_BODY_SIZE, BQ_SPIKE_BODY_SIZE_PCT,
  BQ_SPIKE_UPPER_WICK, BQ_SPIKE_LOWER_WICK, BQ_SPIKE_UPPER_WICK_RATIO, BQ_SPIKE_LOWER_WICK_RATIO,
  BQ_SPIKE_TOTAL_RANGE, BQ_SPIKE_RANGE_PCT, BQ_SPIKE_CLOSE_OPEN_RATIO, BQ_SPIKE_PRICE_MA, BQ_SPIKE_PRICE_ZSCORE,
  BQ_SPIKE_VOLUME_MA, BQ_SPIKE_VOLUME_RATIO, BQ_SPIKE_VOLUME_ZSCORE, BQ_SPIKE_QUOTE_VOLUME_MA,
  BQ_SPIKE_QUOTE_VOLUME_RATIO, BQ_SPIKE_MOMENTUM_3, BQ_SPIKE_MOMENTUM_5, BQ_SPIKE_CLOSE_TO_HIGH,
  BQ_SPIKE_CLOSE_TO_LOW, BQ_SPIKE_STD_RATIO_8_20, BQ_SPIKE_PC_2C, BQ_SPIKE_PC_3C, BQ_SPIKE_PC_POS_COUNT_5,
  BQ_SPIKE_PC_ABS_SUM_5, BQ_SPIKE_BODY_SIZE_PCT_MA_10, BQ_SPIKE_BODY_SIZE_PCT_Z, BQ_NUM_SPIKE_BASE_F
};
enum bq_spike_base_bcol {
  BQ_SPIKE_IS_BULLISH = 0, BQ_SPIKE_VOL_COMPRESSION_FLAG, BQ_SPIKE_UPWARD, BQ_SPIKE_DOWNWARD, BQ_NUM_SPIKE_BASE_B
};
enum bq_spike_flag_fcol {
  BQ_SPIKE_VOL_RATIO_SLOPE_3 = 0, BQ_SPIKE_VOL_RATIO_ACCEL, BQ_SPIKE_PRICE_BREAK_THRESHOLD, BQ_SPIKE_EARLY_PROBA,
  BQ_NUM_SPIKE_FLAG_F
};
enum bq_spike_flag_bcol {
  BQ_SPIKE_VOLUME_CLUSTER_FLAG = 0, BQ_SPIKE_PRICE_BREAK_FLAG, BQ_SPIKE_CUM_BREAK_FLAG, BQ_SPIKE_CUM_BREAK_SHORT_FLAG,
  BQ_SPIKE_ACCEL_FLAG, BQ_SPIKE_ACCEL_SHORT_FLAG, BQ_SPIKE_LABEL_PRE, BQ_SPIKE_LABEL_SHORT_PRE,
  BQ_SPIKE_EARLY_AUG_FLAG, BQ_NUM_SPIKE_FLAG_B
};
int bq_spike_base(const double* const* in, int64_t S, int64_t T, int64_t ld_in, int32_t base_window,
                  int32_t streak_length, double* const* out_f, uint8_t* const* out_b, int64_t ld_out, void* stream);
/*
 * bq_spike_base_std: the same pass in panel mode with the five rolling std
 * columns (FailedSpikeFade.compute_base_features' price_std, volume_std,
 * rolling_price_std_8 / _20 and compute_early_features' body_size_pct std 10,
 * failed_spike_fade.py:293-339) formed in the pass — two-pass window sums
 * (the window's variance to rounding) instead of the bit-exact replay of
 * pandas' online recurrence. in = the first 7 inputs of bq_spike_base
 * {open, high, low, close, volume, quote_volume, ffilled close}; out_sd
 * [BQ_NUM_SPIKE_STD] fp64 [S][ld_out] (NULL entries = not written).
 */
enum bq_spike_std_col {
  BQ_SPIKE_STD_PRICE = 0, BQ_SPIKE_STD_VOLUME, BQ_SPIKE_STD_8, BQ_SPIKE_STD_20, BQ_SPIKE_STD_BODY_PCT_10,
  BQ_NUM_SPIKE_STD
};
int bq_spike_base_std(const double* const* in, int64_t S, int64_t T, int64_t ld_in, int32_t base_window,
                      int32_t streak_length, double* const* out_f, uint8_t* const* out_b, double* const* out_sd,
                      int64_t ld_out, void* stream);
int bq_spike_flags(const double* const* in, const double* vcmr, const double* pbbt, int64_t S, int64_t T,
                   int64_t ld_in, const bq_spike_params* p, double* const* out_f, uint8_t* const* out_b,
                   int64_t ld_out, void* stream);

/* ---- sequential state machines (lane = symbol) ----------------------------- */
/*
 * Supertrend trend flag and final bands (pybinbot Indicators.set_supertrend,
 * called at strategies/coinrule/coinrule.py:143 with multiplier 3.0, period 10;
 * the consumer reads bool(df["supertrend"].iloc[-1]) at :160). hlca = {high,
 * low, close, ATR} [S][ld_in] fp64 (ATR = bq_enrich's ATR column with
 * atr_window = period). up: uint8 [S][ld_out] (1 = uptrend); upper/lower:
 * fp64 [S][ld_out] final bands (NULL = skip). Recurrence: see bq_seq.hip.
 */
int bq_supertrend(const double* const* hlca, int64_t S, int64_t T, int64_t ld_in, double multiplier,
                  uint8_t* up, double* upper, double* lower, int64_t ld_out, void* stream);
/*
 * bq_supertrend with the ATR formed in the same walk: hlc = {high, low, close}
 * [S][ld_in] fp64, ATR = TR.rolling(period).mean() replayed as pandas'
 * roll_mean (1 <= period <= BQ_MAX_WINDOW), so flags and bands are pandas'
 * bit for bit; one launch, no ATR column in HBM (engine.supertrend).
 */
int bq_supertrend_hlc(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in, int32_t period,
                      double multiplier, uint8_t* up, double* upper, double* lower, int64_t ld_out, void* stream);
/*
 * bq_supertrend_hlc in panel mode (engine.supertrend(exact=False)): one
 * workgroup per row, each thread walks a chunk of it from a warm-up, then
 * every chunk start is verified against its predecessor's end state (the
 * rare wrong one re-walked), so the flags and bands equal the sequential
 * recursion on the same ATR; the ATR (TR.rolling(period).mean(), min_periods
 * = period, same-value rule) is a direct window sum per candle, equal to
 * pandas' roll_mean to rounding, not bit for bit. Rows longer than 2048
 * candles run bq_supertrend_hlc.
 */
int bq_supertrend_panel(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in, int32_t period,
                        double multiplier, uint8_t* up, double* upper, double* lower, int64_t ld_out, void* stream);

/* ---- frame plumbing: resample and timestamp joins (ragged rows) ------------ */
/* Timestamps are int64 ms, ascending within a row; lens[s] = valid candles of
 * row s (NULL: all T). */
#define BQ_MAX_RESAMPLE_FIELDS 12
enum bq_agg { BQ_AGG_FIRST = 0, BQ_AGG_LAST = 1, BQ_AGG_MAX = 2, BQ_AGG_MIN = 3, BQ_AGG_SUM = 4 };
/*
 * Candles.resample(df, interval="1h") (producers/context_evaluator.py:403-407,
 * pybinbot): pandas resample(interval, origin="start_day", closed/label left)
 * .agg(...) on the open_time index. bq_resample_count writes the number of
 * bins of each row (first candle's bin .. last candle's bin) to out_lens[S];
 * bq_resample fills out_ts (bin labels, NULL = skip) and out_fields
 * [nfields][S][ld_out] (ld_out >= max out_lens) with per-field aggregation
 * aggs[f] (bq_agg; NaN-skipping, SUM Kahan-compensated like pandas group_sum;
 * empty bins NaN, SUM 0).
 */
int bq_resample_count(const int64_t* ts, const int64_t* lens, int64_t S, int64_t T, int64_t ld_in,
                      int64_t interval_ms, int64_t* out_lens, void* stream);
int bq_resample(const int64_t* ts, const double* const* fields, const int32_t* aggs, int32_t nfields,
                const int64_t* lens, int64_t S, int64_t T, int64_t ld_in, int64_t interval_ms, int64_t* out_ts,
                double* const* out_fields, int64_t ld_out, void* stream);
/* bq_resample for a fixed output geometry (a captured graph sizes ld_out on
 * the host): a row with more bins than ld_out — a gap in the candles widens
 * the span, and pandas emits every empty bin of it — keeps its NEWEST ld_out
 * bins (output bin b = the row's bin b + out_lens[s] - ld_out), so the last
 * written bin is always the row's latest, the one process_data reads. */
int bq_resample_tail(const int64_t* ts, const double* const* fields, const int32_t* aggs, int32_t nfields,
                     const int64_t* lens, int64_t S, int64_t T, int64_t ld_in, int64_t interval_ms, int64_t* out_ts,
                     double* const* out_fields, int64_t ld_out, void* stream);
/*
 * Left merge of a benchmark series on the timestamp
 * (strategies/liquidation_sweep_pump.py:255-263, duplicates keep "last"):
 * out[s][t] = bench_val[j] with bench_ts[j] == ts[s][t], NaN if absent.
 * bench_ts ascending, n_bench entries.
 */
int bq_align(const int64_t* ts, const int64_t* lens, int64_t S, int64_t T, int64_t ld_in, const int64_t* bench_ts,
             const double* bench_val, int64_t n_bench, double* out, int64_t ld_out, void* stream);
/*
 * The aligned returns of ContextEvaluator.dynamic_btc_beta_corr
 * (producers/context_evaluator.py:161-177): log(c/c.shift(1)) on each frame's
 * own rows, inner-joined on the timestamp, dropna'd, compacted in order into
 * x (symbol) / y (benchmark) [S][ld_out] with out_lens[s] pairs (NaN tail).
 * A time the benchmark holds k times joins k pairs, in the benchmark's order,
 * each with the return over the benchmark row before it (pandas' inner join
 * on a repeated right index); a row whose pairs would pass ld_out keeps the
 * first ld_out (out_lens[s] = ld_out). bench_ts ascending.
 */
int bq_join_returns(const int64_t* ts, const double* close, const int64_t* lens, int64_t S, int64_t T, int64_t ld_in,
                    const int64_t* bench_ts, const double* bench_close, int64_t n_bench, double* x, double* y,
                    int64_t ld_out, int64_t* out_lens, void* stream);
/*
 * bq_beta_corr on already-aligned return pairs (x, y [S][ld_in], dropna'd
 * prefix of each row): beta/corr of rolling(window) at every row, NaN for
 * rows < window - 1.
 */
/* bq_beta_corr with the benchmark given as its log returns (btc_returns[T],
 * btc_returns[t] = log(btc[t] / btc[t-1]), NaN at t = 0): the returns are
 * formed once per call instead of once per symbol row (engine.beta_corr).
 * scratch: NULL, or 3*T doubles of device memory in which the benchmark's
 * window mean / variance / inverse variance are computed once (a
 * one-workgroup pre-pass) instead of in every symbol's wave. */
int bq_beta_corr_bret(const double* close, const double* btc_returns, double* scratch, int64_t S, int64_t T,
                      int64_t ld_in, int32_t window, double* beta, double* corr, int64_t ld_out, void* stream);
/* bq_beta_corr with a device scratch of 4*T doubles: a one-workgroup
 * pre-pass forms the benchmark's log returns and their window mean /
 * variance / inverse variance once per call, then one wave per symbol row
 * (engine.beta_corr: two launches per call, no host-side returns pass). */
int bq_beta_corr_ws(const double* close, const double* btc_close, double* scratch, int64_t S, int64_t T,
                    int64_t ld_in, int32_t window, double* beta, double* corr, int64_t ld_out, void* stream);
int bq_beta_corr_pairs(const double* x, const double* y, int64_t S, int64_t T, int64_t ld_in, int32_t window,
                       double* beta, double* corr, int64_t ld_out, void* stream);

/* ---- device-resident MarketStateStore -------------------------------------- */
/*
 * market_regime/market_state_store.py:14-87 kept in HBM: per symbol slot a
 * ring of the last max_bars closed candles, sorted by timestamp, unique
 * timestamps (a later update of a timestamp replaces it, keep="last").
 * Caller-owned buffers (the library allocates nothing):
 */
#define BQ_STORE_MAX_BARS 512
typedef struct bq_store_view {
  int64_t* ts;                     /* [capacity][max_bars] candle timestamps (ms)        */
  double*  field[BQ_NUM_INPUTS];   /* open, high, low, close, volume, same layout       */
  int32_t* head;                   /* [capacity] ring index of the oldest candle        */
  int32_t* count;                  /* [capacity] candles held (<= max_bars)             */
  int64_t* last;                   /* [capacity] last closed timestamp (undefined if 0) */
  int64_t  capacity;
  int32_t  max_bars;               /* 2 .. BQ_STORE_MAX_BARS                            */
  int32_t  reserved;
} bq_store_view;
/*
 * MarketStateStore.update for a batch: n_seg runs of candles, run g =
 * [seg_begin[g], seg_begin[g+1]) all for slot[seg_begin[g]], timestamps
 * strictly ascending inside a run, one run per slot per call (the caller
 * sorts and de-duplicates the batch, keep="last"). NaN close / timestamp rows
 * must already be dropped (market_state_store.py:84). slot, ts, seg_begin and
 * the five ohlcv arrays are device pointers.
 */
int bq_store_update(const bq_store_view* st, const int64_t* slot, const int64_t* ts, const double* const* ohlcv,
                    const int64_t* seg_begin, int64_t n_seg, void* stream);
/*
 * LiveMarketContextAccumulator._compute_symbol_features
 * (market_regime/live_market_context_accumulator.py:244-297) on the histories
 * of n_sel slots: feat[BQ_NUM_FEATURES] arrays of n_sel doubles (NULL =
 * skip; NaN rows where a history has < 2 candles, i.e. the reference's None)
 * and close_out[n_sel] (latest close). pandas' ewm / roll_mean / roll_var
 * recurrences are replayed, so values equal pandas' bit for bit.
 */
int bq_store_features(const bq_store_view* st, const int64_t* slots, int64_t n_sel, double* const* feat,
                      double* close_out, void* stream);
/*
 * The per-symbol pass of one live context build
 * (LiveMarketContextAccumulator._build_context,
 * market_regime/live_market_context_accumulator.py:95-133) over ALL n tracked
 * slots [0, n): a slot is fresh when its last closed candle is *fresh_ts
 * (MarketStateStore.get_fresh_symbols, market_state_store.py:49-54; fresh_ts
 * is a device pointer, so a captured graph reads the tick's timestamp).
 * feat / close_out rows: the features of counted fresh slots, NaN otherwise
 * (the benchmark's row only when btc_counted: a sharded store replicates the
 * benchmark and counts it on one rank); fresh_out[n]: 1.0 / 0.0 for those
 * rows; btc_out[8]: the benchmark's features, latest close (whatever its
 * freshness, :105-106) and 1.0 / 0.0 = fresh (unwritten when btc_slot < 0). Same replay as
 * bq_store_features (pandas bit for bit); non-fresh slots are not replayed.
 */
int bq_store_context_features(const bq_store_view* st, int64_t n, const int64_t* fresh_ts, int64_t btc_slot,
                              int btc_counted, double* const* feat, double* close_out, double* fresh_out,
                              double* btc_out, void* stream);
/*
 * MarketStateStore.get_symbol_history / get_all_histories: time-ordered copy
 * of n_sel slots into ts_out / out[BQ_NUM_INPUTS] [n_sel][ld_out]
 * (ld_out >= max_bars; NaN / 0 past each slot's count; NULL = skip).
 */
int bq_store_gather(const bq_store_view* st, const int64_t* slots, int64_t n_sel, int64_t* ts_out,
                    double* const* out, int64_t ld_out, void* stream);

/* ---- signal-generator helpers, time-parallel (bq_signals.hip) --------------- */
/*
 * The inline helpers of the signal generators at every candle of a [S][T]
 * panel (column t = the helper on df.iloc[:t + 1]), split along the time axis
 * (tolerance-exact, 1e-9 relative; the bit-exact replay of the same helpers is
 * the binquant_amd.signals composition with exact=True). Finite prices in,
 * out [S][ld_out] fp64 device pointers.
 *   bq_wilder_rsi  MeanReversionFade._rsi (strategies/mean_reversion_fade.py:88-109):
 *                  ewm(alpha=1/window, min_periods=window, adjust=False) of
 *                  gains / losses, 100 g / (g + l), 50 where g + l == 0
 *   bq_zscore      RangeBbRsiMeanReversion._compute_zscore
 *                  (strategies/range_bb_rsi_mean_reversion.py:132-138): 0 where
 *                  the ddof-0 std is 0 or NaN (warm-up included)
 *   bq_adx         RangeBbRsiMeanReversion._compute_adx (:101-130): 100 where
 *                  the window mean of dx is NaN; window <= 64
 */
int bq_wilder_rsi(const double* close, int64_t S, int64_t T, int64_t ld_in, int32_t window, double* out,
                  int64_t ld_out, void* stream);
int bq_zscore(const double* close, int64_t S, int64_t T, int64_t ld_in, int32_t window, double* out, int64_t ld_out,
              void* stream);
int bq_adx(const double* high, const double* low, const double* close, int64_t S, int64_t T, int64_t ld_in,
           int32_t window, double* out, int64_t ld_out, void* stream);

/* ---- regime annotation, candidate scoring, portfolio selection -------------- */
enum bq_micro_regime_code {   /* models.py:15-21 MicroRegime; -1 = None */
  BQ_MICRO_TREND_UP = 0, BQ_MICRO_TREND_DOWN = 1, BQ_MICRO_RANGE = 2, BQ_MICRO_VOLATILE = 3,
  BQ_MICRO_TRANSITIONAL = 4
};
enum bq_micro_transition_code {   /* models.py:32-42 MicroRegimeTransition; -1 = None */
  BQ_MT_VOLATILITY_EXPANSION = 0, BQ_MT_BREAKOUT_UP, BQ_MT_BREAKDOWN, BQ_MT_RECOVERY, BQ_MT_MEAN_REVERSION,
  BQ_MT_ENTERED_TREND_UP, BQ_MT_ENTERED_TREND_DOWN, BQ_MT_ENTERED_RANGE, BQ_MT_ENTERED_TRANSITIONAL
};
/*
 * RegimeTransitionDetector._annotate_symbol_regime (market_regime/regime_transitions.py:162-232)
 * for n symbols: device arrays of the SymbolMarketFeatures fields; prev_regime
 * (int8, -1 = None; NULL = no previous context) / prev_strength chain the
 * transition. Outputs regime/strength (+ transition / transition_strength,
 * NULL = skip). Bit-exact with the Python floats.
 */
int bq_micro_regime(int64_t n, const double* trend, const uint8_t* above_ema20, const uint8_t* above_ema50,
                    const double* rs, const double* bb_width, const double* atr_pct, const double* return_pct,
                    const int8_t* prev_regime, const double* prev_strength, int8_t* regime, double* strength,
                    int8_t* transition, double* transition_strength, void* stream);

/*
 * The per-symbol regime panel: for every candle t of a [S][T_out] panel, the
 * symbol_features entry of symbol s in the market context that candle saw
 * (KlinesProvider.latest_market_context + resolve_symbol_features), with the
 * micro regime and transition of RegimeTransitionDetector.annotate_context
 * (regime_transitions.py:25-43, :162-232) against the context stored
 * immediately before the seen one. One streaming pass; stream-ordered; no
 * atomics (bitwise reproducible).
 *
 * feat[BQ_NUM_FEATURES] [S][ld_f] and close [S][ld_c]: the feature columns of
 * a context build and the close they were computed from, Tc columns each.
 * rank: NULL (dense build: symbol s has features at context column j iff
 * j >= 1, its feature column is j) or [S][ld_r] int32 of a fresh build
 * (bq_panel_compact: with k = rank[s][j] the symbol has features iff k >= 1,
 * its feature column is k; feat / close are then the packed ones).
 * at[T_out] int32: the context column candle t sees, negative for none.
 * prev[T_out] int32: the context column stored before at[t]; -1 none, -2 the
 * seed (seed_regime int8 [S], negative = None, and seed_strength [S]; either
 * may be NULL: None / 0.0). btc_return[Tc]: BTC's return_pct in context
 * column j, NaN where BTC has no features (every rs is then 0.0); btc_row:
 * BTC's row (its own rs stays 0.0) or -1.
 *
 * out_u8[BQ_RP_NUM_U8] [S][ld_u8] and out_f64[BQ_RP_NUM_F64] [S][ld_f64], in
 * the enums' order; a NULL entry is neither computed nor written. Where the
 * symbol has no features in the seen context (or no context is seen): ok 0,
 * the codes 255, the flags 0, the values NaN. micro_regime / micro_transition
 * index bq_micro_regime_code / bq_micro_transition_code (255 = None).
 * Tc, T_out <= 2^31 - 257; S * ceil(T_out / 256) <= 2^31 - 1.
 */
enum bq_regime_panel_u8 {
  BQ_RP_OK = 0, BQ_RP_MICRO_REGIME, BQ_RP_MICRO_TRANSITION, BQ_RP_ABOVE_EMA20, BQ_RP_ABOVE_EMA50, BQ_RP_NUM_U8
};
enum bq_regime_panel_f64 {
  BQ_RP_RS_VS_BTC = 0, BQ_RP_REGIME_STRENGTH, BQ_RP_TRANSITION_STRENGTH, BQ_RP_TREND_SCORE, BQ_RP_ATR_PCT,
  BQ_RP_BB_WIDTH, BQ_RP_NUM_F64
};
int bq_symbol_regime_panel(const double* const* feat, int64_t ld_f, const double* close, int64_t ld_c,
                           const int32_t* rank, int64_t ld_r, int64_t S, int64_t Tc, const int32_t* at,
                           const int32_t* prev, int64_t T_out, const double* btc_return, int64_t btc_row,
                           const int8_t* seed_regime, const double* seed_strength, uint8_t* const* out_u8,
                           int64_t ld_u8, double* const* out_f64, int64_t ld_f64, void* stream);

enum bq_direction { BQ_DIR_LONG = 0, BQ_DIR_SHORT = 1, BQ_DIR_OTHER = 2 };   /* direction.upper().strip() */
typedef struct bq_context_scalars {   /* the LiveMarketContext fields the scorer reads */
  double confidence, long_tailwind, short_tailwind, btc_regime_score, market_stress_score;
  int32_t present;                    /* 0: no context (None) */
  int32_t reserved;
} bq_context_scalars;
typedef struct bq_scorer_weights {    /* SignalContextScorer (signal_context_scorer.py:10-13) */
  double context_weight, risk_weight, support_weight;
} bq_scorer_weights;
enum bq_score_field {   /* MarketContextScore fields + the adjusted score; out[field][ld_out] */
  BQ_SC_CONFIDENCE = 0, BQ_SC_BREADTH, BQ_SC_BTC_ALIGNMENT, BQ_SC_CROSS_ASSET, BQ_SC_FOLLOWTHROUGH,
  BQ_SC_ADVERSE, BQ_SC_OVERRIDE, BQ_SC_SUPPORTIVENESS, BQ_SC_ADJUSTED, BQ_NUM_SCORE_FIELDS
};
/*
 * RuleBasedMarketContextModel.evaluate (market_regime/context_scoring.py:13-114)
 * + SignalContextScorer.adjust_score (signal_context_scorer.py:15-28) for n
 * candidates against one context: direction (bq_direction), rs / trend (the
 * candidate's local_features or its snapshot row, resolved by the caller),
 * local_score (NULL = 0). out: BQ_NUM_SCORE_FIELDS x ld_out doubles.
 */
int bq_context_score(int64_t n, const int8_t* direction, const double* rs, const double* trend,
                     const double* local_score, const bq_context_scalars* ctx, const bq_scorer_weights* weights,
                     double* out, int64_t ld_out, void* stream);
/*
 * Portfolio winners (strategies/liquidation_sweep_pump.py:38-87,
 * strategies/gradual_gainer_retest.py:33-70): per cohort (dense ids
 * 0..n_cohorts-1) the accepted candidate (accepted NULL = all) with the
 * largest (score, symbol_rank), the latest submission on a full tie.
 * winner[n_cohorts]: candidate index or -1. scratch: 2*n_cohorts u64 (device).
 */
int bq_cohort_select(int64_t n, const int32_t* cohort, const uint8_t* accepted, const double* score,
                     const int32_t* symbol_rank, int32_t n_cohorts, unsigned long long* scratch, int64_t* winner,
                     void* stream);

/* ---- wire-format ingest (host) ------------------------------------------------ */
/*
 * Binance kline websocket events (one JSON object per '\n'-separated frame,
 * as decoded at producers/klines_connector.py:77-90 and copied into a
 * KlineProduceModel at :148-164) -> arrays, in one native pass: sym
 * [max_rows][sym_stride] NUL-terminated symbols ("s"), open_time ("t"),
 * close_time ("T"), ohlcv[5] ("o","h","l","c","v" via strtod: the same
 * doubles as Python float()), closed ("x"). HOST pointers. Non-kline frames
 * are skipped; malformed kline frames are counted in n_bad and skipped.
 * Returns BQ_EINVAL (with n_rows filled so far) if max_rows is too small.
 */
int bq_parse_kline_events(const char* buf, int64_t len, int64_t max_rows, char* sym, int64_t sym_stride,
                          int64_t* open_time, int64_t* close_time, double* const* ohlcv, uint8_t* closed,
                          int64_t* n_rows, int64_t* n_bad);

/* ---- fused element-wise programs ---------------------------------------------- */
/*
 * The element-wise glue of the strategy pipelines (SURVEY §8a a17-a20:
 * ratios, clips, flags, shifted differences, where-selections between the
 * rolling series — e.g. activity_burst_pump.py:64-133, liquidation_sweep_pump.py:
 * 218-269, failed_spike_fade.py:260-493) evaluated as ONE launch per stage: a
 * straight-line program run per element (s, t) of an [S, T] panel, values in
 * fp64 with IEEE operations in the order the program lists them (the
 * reference's pandas operation order), so results equal the unfused
 * arithmetic bit for bit. Intermediates live in LDS registers, never in HBM.
 *
 * Instruction (uint64): op | dst << 8 | a << 16 | b << 24 | c << 32 | imm << 40
 * (imm: signed 24-bit). The first n_loads instructions are BQ_F_LD, issued
 * together before the rest runs.
 *   LD      dst <- in[b] at t - imm (consts[c] when t - imm is outside [0, T))
 *   CONST   dst <- consts[imm];   INRANGE dst <- 0 <= t - imm < T
 *   binary  dst <- a (op) b;      unary dst <- (op) a
 *   WHERE   dst <- a != 0 ? b : c
 *   (operand k of these ops is consts[k-th index] instead of a register
 *   when bit k of imm is set)
 *   ST      out[imm] <- a (BQ_F_U8 outputs store a != 0)
 * Comparisons give 1.0 / 0.0 (NaN compares false); AND / OR / NOT treat
 * non-zero as true; FMAX / FMIN skip NaN (torch.fmax), MAXIMUM / MINIMUM
 * propagate it (torch.maximum).
 * Operands: element (s, t) at ptr + s * stride_s + t * stride_t elements
 * (stride_t 0: a per-symbol value; stride_s 0: one series for all symbols).
 */
#define BQ_FUSED_MAX_INS 192
#define BQ_FUSED_MAX_CONST 32
#define BQ_FUSED_MAX_IN 16
#define BQ_FUSED_MAX_OUT 24
#define BQ_FUSED_MAX_REGS 20
#define BQ_FUSED_MAX_LOADS 16

enum bq_fused_dtype { BQ_F_F64 = 0, BQ_F_U8 = 1 };

enum bq_fused_op {
  BQ_F_LD = 1, BQ_F_CONST = 2, BQ_F_INRANGE = 3,
  BQ_F_ADD = 4, BQ_F_SUB = 5, BQ_F_MUL = 6, BQ_F_DIV = 7,
  BQ_F_FMAX = 8, BQ_F_FMIN = 9, BQ_F_MAXIMUM = 10, BQ_F_MINIMUM = 11,
  BQ_F_GT = 12, BQ_F_GE = 13, BQ_F_LT = 14, BQ_F_LE = 15, BQ_F_EQ = 16, BQ_F_NE = 17,
  BQ_F_AND = 18, BQ_F_OR = 19, BQ_F_NOT = 20,
  BQ_F_ABS = 21, BQ_F_NEG = 22, BQ_F_ISNAN = 23, BQ_F_SQRT = 24, BQ_F_LOG = 25,
  BQ_F_WHERE = 26, BQ_F_ST = 27
};

typedef struct {
  const void* ptr;
  int64_t stride_s, stride_t;   /* in elements */
  int32_t dtype;                /* bq_fused_dtype */
  int32_t reserved;
} bq_fused_operand;

typedef struct {
  int32_t n_ins, n_loads, n_regs, n_in, n_out, n_const;
  uint64_t ins[BQ_FUSED_MAX_INS];
  double consts[BQ_FUSED_MAX_CONST];
  bq_fused_operand in[BQ_FUSED_MAX_IN];
  bq_fused_operand out[BQ_FUSED_MAX_OUT];
} bq_fused_program;

/* Validates the program (opcodes, register / operand / constant indices,
 * loads first) and runs it over the [S, T] panel. Device operand pointers. */
int bq_fused_eval(const bq_fused_program* prog, int64_t S, int64_t T, void* stream);

/* Native form of the same programs: bq_fused_eval translates the program into
 * straight-line HIP source (operand layouts specialised, constants as exact
 * bit patterns), compiles it for gfx950 with hiprtc on first use and launches
 * the compiled kernel — bit-identical to the interpreter (the default; the
 * environment variable BQ_FUSED_NATIVE=0 or bq_fused_set_native(0) selects
 * the interpreter, -1 restores the environment's choice; returns the previous
 * setting, -1 if unset). Compiled code objects are cached per process and,
 * if a directory is set, on disk (<dir>/<hash>.gfx950.co + its source). */
int bq_fused_set_native(int on);
int bq_fused_set_cache_dir(const char* dir);
/* generated source of a (validated) program: *len = its length; up to cap-1
 * bytes + NUL copied into buf when buf is non-null. No device needed. */
int bq_fused_source(const bq_fused_program* prog, char* buf, int64_t cap, int64_t* len);
/* compile (or find in the caches) without launching. No device needed. */
int bq_fused_compile(const bq_fused_program* prog);
/* counters: hiprtc compiles, disk-cache hits, programs in the process cache */
int bq_fused_stats(int64_t* compiles, int64_t* disk_hits, int64_t* cached);

#ifdef __cplusplus
}
#endif

#endif /* BINQUANT_AMD_H */
