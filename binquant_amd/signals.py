"""Batched inline indicator helpers of the signal generators.

The reference's strategies compute a handful of small indicators inline on one
symbol's frame and read the last row(s). Here every helper evaluates the whole
[S, T] panel on the device, so column t is what the reference returns for the
prefix frame df.iloc[:t + 1]:

* wilder_rsi         MeanReversionFade._rsi (strategies/mean_reversion_fade.py:88-109)
* trend_score        MeanReversionFade._trend_score (:149-155), also the EMA9/21
                     trend of strategies/coinrule/price_tracker.py:204-211
* ema                close.ewm(span, adjust=False, min_periods) as used by
                     price_tracker.py:204-205, top_gainer_early_momentum.py:153-154,
                     gradual_gainer_retest.py:257-259 (read at t-1),
                     coinrule/buy_the_dip.py:63-71 (min_periods=1)
* adx, zscore        RangeBbRsiMeanReversion._compute_adx / _compute_zscore
                     (strategies/range_bb_rsi_mean_reversion.py:101-138)
* top_gainer_features TopGainerEarlyMomentum._features
                     (strategies/top_gainer_early_momentum.py:92-160)
* mean_reversion_features  the entry inputs of MeanReversionFade (:240-255)
* mean_reversion_fade_entry  the decisions of MeanReversionFade.signal()
                     (strategies/mean_reversion_fade.py:224-300) on the 15m
                     frame: RSI hook and rolling means formed in the pass,
                     _resolve_entry, the trend ceiling, the SHORT risk
                     profile, once per candle, the stop-loss cap, one pass
                     (bq_meanrev.hip)
* range_fade_entry   the decisions of RangeBbRsiMeanReversion.signal()
                     (strategies/range_bb_rsi_mean_reversion.py:202-274) on the
                     15m frame: null gate, regime_routing, ADX and z-score
                     formed in the pass, the two band rejections, local_score,
                     one pass (bq_rangefade.hip)
* impulse_rider_features   RelativeStrengthImpulseRider._features
                     (strategies/relative_strength_impulse_rider.py:92-198), one
                     pass (bq_impulse.hip)
* bb_width_stable    LadderDeployer._bb_stable (strategies/grid/ladder_deployer.py:42-56),
                     one pass (bq_impulse.hip)
* gradual_gainer_retest    the body of GradualGainerRetest.signal()
                     (strategies/gradual_gainer_retest.py:222-308): the watchlist
                     state machine replayed per row (bq_retest.hip), with
                     retest_risk_allows for _risk_allows (:198-215)
* top_gainer_entry   TopGainerEarlyMomentum's _features, _entry_allows and
                     signal()'s two-close confirmation
                     (strategies/top_gainer_early_momentum.py:91-253, :363-406),
                     one pass (bq_topgainer.hip), with top_gainer_risk_allows
                     for _risk_profile_allows (:204-234)
* failed_spike_fade  the body of FailedSpikeFade.signal()
                     (strategies/failed_spike_fade.py:596-695): the pending-spike
                     state machine replayed per row (bq_spikefade.hip), with
                     spike_source_allows (:190-203), spike_source_frames
                     (that gate on the frame ending at every candle) and
                     spike_fade_market_allows (:155-188)
* price_tracker_entry  the decisions of PriceTracker.signal()
                     (strategies/coinrule/price_tracker.py:165-251) on the 5m
                     frame: null gate, oversold test, local and context
                     score, the three rejections and the entry cooldown, one
                     pass (bq_pricetracker.hip), with price_tracker_routing
                     for regime_routing (:113-163)
* activity_burst_entry  ActivityBurstPump.signal()'s frame gate, routing and
                     qualified_signal (strategies/activity_burst_pump.py:160-185),
                     with long_autotrade_allows for allows_long_autotrade
                     (market_regime/regime_routing.py:30-75)
* buy_the_dip_entry  the decisions of BuyTheDip.signal()
                     (strategies/coinrule/buy_the_dip.py:127-181) on the 15m
                     frame: null gate, start time, the 6 h reference candle
                     found by close_time, the change band, _allows_entry and
                     the prior-close / EMA20 reclaim, one pass (bq_dip.hip),
                     with buy_the_dip_routing for the message's autotrade flag
                     and route (:87-125)
* rs_reversal_entry  the decisions of RelativeStrengthReversalRange.signal()
                     (strategies/relative_strength_reversal_range.py:56-101)
                     on the 15m frame: the frame gate, regime_routing and
                     the 24 h volume floor (Series.quantile, sorted only
                     where a candle passes the route), one pass
                     (bq_rsreversal.hip)
* grid_ladder_entry  the decisions of LadderDeployer.signal()
                     (strategies/grid/ladder_deployer.py:58-187) on the 15m
                     frame: the policy, context and symbol gates, _bb_stable,
                     the price and width tests, and the deployment's
                     range_width_pct, breakout buffer and breakout_low / high,
                     one pass (bq_ladder.hip), with grid_only_policy for
                     GridOnlyPolicy.resolve (market_regime/grid_only_policy.py
                     :121-158)

wilder_rsi, zscore and adx default to the time-parallel kernels of
bq_signals.hip (one launch each, 1e-9 of pandas); exact=True runs the
replay composition instead — the bq_rolling / bq_ewm kernels plus fused
element-wise programs (binquant_amd.fused) in the reference's operation
order, equal to pandas bit for bit. The other helpers use that composition.
Rows with missing candles (NaN) keep pandas' NaN rules on the fast kernels
too (bq_signals.hip: z-score / ADX re-sum the windows a gap touched; the
Wilder RSI row is replayed with pandas' own ewm update from the first gap).
There is no CPU path.
"""

from __future__ import annotations

import torch

from . import _lib, engine
from . import fused as F

NAN = float("nan")

# TopGainerEarlyMomentum._features status strings, as int8 codes
TG_READY, TG_SHORT_HISTORY, TG_INVALID_CANDLE, TG_NOT_READY = 0, 1, 2, 3
TG_STATUS = {TG_READY: "features_ready", TG_SHORT_HISTORY: "history_too_short",
             TG_INVALID_CANDLE: "invalid_candle_values", TG_NOT_READY: "indicators_not_ready"}
TG_KEYS = ("close", "open", "high", "low", "volume", "quote_volume", "previous_high", "return_1h", "return_2h",
           "return_6h", "extension_return", "extension_window_bars", "extension_cap", "candle_return",
           "volume_ratio", "quote_volume_ratio", "range_position", "upper_wick_fraction", "ema20", "ema50", "atr")


def ema(close: torch.Tensor, span: int, min_periods: int = 0) -> torch.Tensor:
    """close.ewm(span=span, adjust=False, min_periods=min_periods).mean()."""
    return engine.ewm(close, span=span, min_periods=min_periods)


def _rsi_ex(close: torch.Tensor, window: int) -> F.Ex:
    C = F.inp(close)
    delta = F.diff(C, 1)
    g = F.run({"g": F.clip_lower(delta, 0.0), "l": -F.where(delta > 0, 0.0, delta)})   # -delta.clip(upper=0)
    ag, al = engine.rolling_many(engine.Ewm(g["g"], alpha=1 / window, min_periods=window),
                                 engine.Ewm(g["l"], alpha=1 / window, min_periods=window))
    AG = F.inp(ag)
    den = AG + al
    return F.where(den != 0, 100 * AG / den, 50.0)


def wilder_rsi(close: torch.Tensor, window: int = 14, exact: bool = False) -> torch.Tensor:
    """Wilder RSI: ewm(alpha=1/window, min_periods=window, adjust=False) of
    gains/losses, 100*g/(g+l), 50 where g+l == 0 (NaN warm-up kept)."""
    if not exact:
        return engine.wilder_rsi(close, window)
    return F.run({"rsi": _rsi_ex(close, window)})["rsi"]


def _trend_ex(close: torch.Tensor, fast: int, slow: int) -> F.Ex:
    f, s = engine.rolling_many(engine.Ewm(close, span=fast), engine.Ewm(close, span=slow))
    Fx, Sx = F.inp(f), F.inp(s)
    return F.where(Sx == 0, 0.0, (Fx - Sx) / Sx.abs())


def trend_score(close: torch.Tensor, fast: int = 20, slow: int = 50) -> torch.Tensor:
    """(ema_fast - ema_slow) / |ema_slow|, 0 where ema_slow == 0."""
    return F.run({"t": _trend_ex(close, fast, slow)})["t"]


def adx(high: torch.Tensor, low: torch.Tensor, close: torch.Tensor, window: int = 14,
        exact: bool = False) -> torch.Tensor:
    """_compute_adx at every t: rolling-sum DI+/DI-, dx NaN -> 0, mean over
    `window`; NaN (short history) -> 100."""
    if not exact and window <= 64:
        return engine.adx(high, low, close, window)
    H, L, C = F.inp(high), F.inp(low), F.inp(close)
    hd = F.diff(H, 1)
    ld = -F.diff(L, 1)
    pc = F.shift(C, 1)
    dm = F.run({
        "tr": F.fmax(F.fmax(H - L, (H - pc).abs()), (L - pc).abs()),   # max(axis=1) skips NaN
        "plus": F.where((hd > ld) & (hd > 0), hd, 0.0),
        "minus": F.where((ld > hd) & (ld > 0), ld, 0.0),
    })
    atr_sum, plus_sum, minus_sum = engine.rolling_many(
        engine.Roll(dm["tr"], window, "sum"), engine.Roll(dm["plus"], window, "sum"),
        engine.Roll(dm["minus"], window, "sum"))
    A = F.inp(atr_sum)
    plus_di = 100.0 * F.inp(plus_sum) / A
    minus_di = 100.0 * F.inp(minus_sum) / A
    total = plus_di + minus_di
    dx = 100.0 * (plus_di - minus_di).abs() / F.where(total != 0, total, NAN)
    dx = F.run({"dx": F.fillna(dx, 0.0)})["dx"]
    a = engine.rolling(dx, window, "mean")
    return F.run({"adx": F.fillna(a, 100.0)})["adx"]


def zscore(close: torch.Tensor, window: int = 20, exact: bool = False) -> torch.Tensor:
    """_compute_zscore at every t: (c - mean) / std(ddof=0); 0 where std is 0
    or NaN."""
    if not exact:
        return engine.zscore(close, window)
    mean, std = engine.rolling_many(engine.Roll(close, window, "mean"), engine.Roll(close, window, "std0"))
    SD = F.inp(std)
    bad = (SD == 0) | F.isnan(SD)
    return F.run({"z": F.where(bad, 0.0, (F.inp(close) - mean) / SD)})["z"]


def top_gainer_features(o, h, l, c, v, qv=None, atr=None, min_history: int = 56, lookback_high: int = 48,
                        volume_window: int = 32, full_extension_bars: int = 96, max_extension: float = 0.50,
                        min_short_extension_cap: float = 0.25):
    """TopGainerEarlyMomentum._features evaluated at every t (prefix frames).
    Returns (values, status): values maps TG_KEYS to [S, T] float64 (NaN where
    status != TG_READY), status is [S, T] int8 (TG_* codes)."""
    S, T = c.shape
    dev = c.device
    eps = 1e-6
    R, E = engine.Roll, engine.Ewm
    # df["high"].iloc[-49:-1].max(): the 48 highs before t (fewer when short; nan-skipping)
    specs = [R(v, volume_window, "mean"), R(h, lookback_high, "max", min_periods=1, shift=1), E(c, span=20),
             E(c, span=50)]
    if qv is not None:
        specs.append(R(qv, volume_window, "mean"))
    res = engine.rolling_many(*specs)
    vma, prev_high, e20, e50 = res[:4]
    qvma = res[4] if qv is not None else None
    C, O, H, L, V = (F.inp(x) for x in (c, o, h, l, v))
    QV = F.inp(qv) if qv is not None else V * C
    QVMA = F.inp(qvma) if qv is not None else F.inp(vma) * C
    # close.iloc[-k - 1] of the prefix frame (t + 1 rows) is close[t - k]; rows
    # with t < k are history_too_short (min_history > 24), masked below
    t = torch.arange(T, device=dev, dtype=torch.int64)
    anchor = torch.clamp(t - full_extension_bars, min=0)
    bars = (t - anchor).to(torch.float64)
    short_cap = torch.clamp(max_extension * (bars / full_extension_bars), min=min_short_extension_cap)
    cap = torch.where(bars < full_extension_bars, short_cap, torch.full_like(bars, max_extension))
    BARS, CAP = F.inp(bars), F.inp(cap)
    # close at the anchor: close[t - 96], or the first close while t < 96
    c_anchor = F.where(BARS < full_extension_bars, F.inp(c[:, :1]), F.shift(C, full_extension_bars))
    rng = H - L
    ex = {
        "close": C, "open": O, "high": H, "low": L, "volume": V, "quote_volume": QV,
        "previous_high": F.inp(prev_high),
        "return_1h": C / F.shift(C, 4) - 1,
        "return_2h": C / F.shift(C, 8) - 1,
        "return_6h": C / F.shift(C, 24) - 1,
        "extension_return": C / c_anchor - 1,
        "extension_window_bars": BARS,
        "extension_cap": CAP,
        "candle_return": C / O - 1,
        "volume_ratio": V / (F.inp(vma) + eps),
        "quote_volume_ratio": QV / (QVMA + eps),
        "range_position": (C - L) / (rng + eps),
        "upper_wick_fraction": (H - F.maximum(O, C)) / (rng + eps),
        "ema20": F.inp(e20),
        "ema50": F.inp(e50),
        "atr": F.inp(atr) if atr is not None else F.const(0.0),
    }
    # status: not finite -> NOT_READY, then python min() <= 0 -> INVALID, then short history
    finite = None
    for k in TG_KEYS:
        x = ex[k]
        ok = ~F.isnan(x - x)          # x - x is NaN for NaN and +-inf
        finite = ok if finite is None else finite & ok
    mn = F.minimum(F.minimum(F.minimum(C, O), F.minimum(H, L)), V)
    invalid = ~(mn > 0) & ~F.isnan(mn)
    short = F.inp(t.to(torch.float64)) < float(min_history - 1)   # len(prefix) = t + 1 < min_history
    code = F.where(short, float(TG_SHORT_HISTORY),
                   F.where(invalid, float(TG_INVALID_CANDLE), F.where(finite, float(TG_READY), float(TG_NOT_READY))))
    status_f = F.run({"status": code}, S, T)["status"]
    ready = F.inp(status_f) == float(TG_READY)
    out = F.run({k: F.where(ready, ex[k], NAN) for k in TG_KEYS}, S, T)
    return out, status_f.to(torch.int8)


_LEADERSHIP_FUSED = True   # False: the staged pipeline for every parameter set (tests)


def gradual_gainer_leadership(open_time: torch.Tensor, close: torch.Tensor, btc_time: torch.Tensor,
                              btc_close: torch.Tensor, rs_quantile: float = 0.80, rs_lookback: int = 96,
                              min_history: int = 100, min_count: int = 20, short: int = 8, long: int = 24):
    """GradualGainerRetest._leadership_allows at every t (column t = the
    method on the prefix frame df.iloc[:t + 1]; strategies/gradual_gainer_retest.py
    :131-196), against the benchmark frame (btc_time ascending, duplicates:
    the later row wins, as the reference's dict does).

    * btc close at each candle's open_time: the left merge bq_align;
    * _relative_strengths: all of the last short·3+1 = 25 times present in the
      benchmark and every close > 0 (a rolling(25) integer sum of that flag),
      rs_2h / rs_6h = c/c[-8] - b/b[-8], c/c[-24] - b/b[-24];
    * the history: one entry per position i >= 24 of the last 96 whose times i,
      i-8, i-24 are all in the benchmark with the six closes > 0 — NaN
      elsewhere, so the 80th-percentile threshold sorted(h)[int((n-1) q)] is
      rolling(96, min_periods=20).quantile(q, interpolation="lower")
      (bq_rolling_batch, BQ_ROLL_QLOWER; order statistics by bit selection);
    * leader = rs_2h > 0 and rs_6h > 0 and rs >= threshold for both.

    Returns {"leader": bool [S, T], "rs_2h": [S, T], "rs_6h": [S, T]} with the
    method's fall-backs: (False, 0.0, 0.0) when the strengths are None or the
    frame is shorter than min_history, (False, rs_2h, rs_6h) when fewer than
    min_count history entries exist.

    The strategy's lookback runs in one pass (engine.leadership,
    bq_leadership); any others run the staged pipeline below. A NaN close is
    not > 0 here, so it never enters the history or the strengths; the
    reference's Python min(...) skips a NaN unless it is its first argument
    (:148, :178) and can append NaN strengths, whose place in sorted() is
    undefined: frames with missing closes are parity-unpinned (the golden
    frames hold none; pre_process drops such rows before the strategies)."""
    fused = engine.leadership(open_time, close, btc_time, btc_close, rs_quantile, rs_lookback, min_history,
                              min_count, short, long) if _LEADERSHIP_FUSED else None
    if fused is not None:   # the strategy's lookback: one pass (bq_leadership)
        return fused
    # any other parameters: the staged pipeline
    S, T = close.shape
    recent = long + 1
    b = engine.align(open_time, btc_time, btc_close)
    C, B = F.inp(close), F.inp(b)
    pos = ((C > 0) & (F.shift(C, short) > 0) & (F.shift(C, long) > 0)
           & (B > 0) & (F.shift(B, short) > 0) & (F.shift(B, long) > 0))
    rs2 = C / F.shift(C, short) - B / F.shift(B, short)
    rs6 = C / F.shift(C, long) - B / F.shift(B, long)
    st = F.run({"h2": F.where(pos, rs2, NAN), "h6": F.where(pos, rs6, NAN),
                "ok": F.where((C > 0) & (B > 0), 1.0, 0.0), "rs2": rs2, "rs6": rs6}, S, T)
    R = engine.Roll
    thr2, thr6, okn = engine.rolling_many(
        R(st["h2"], rs_lookback, "qlower", q=rs_quantile, min_periods=min_count),
        R(st["h6"], rs_lookback, "qlower", q=rs_quantile, min_periods=min_count),
        R(st["ok"], recent, "isum", min_periods=recent))
    n = torch.arange(1, T + 1, device=close.device, dtype=torch.float64)
    R2, R6, T2, T6 = F.inp(st["rs2"]), F.inp(st["rs6"]), F.inp(thr2), F.inp(thr6)
    strengths = (F.inp(okn) == float(recent)) & (F.inp(n) >= float(min_history))
    leader = strengths & ~F.isnan(T2) & (R2 > 0) & (R6 > 0) & (R2 >= T2) & (R6 >= T6)
    res = F.run({"leader": leader, "rs_2h": F.where(strengths, R2, 0.0), "rs_6h": F.where(strengths, R6, 0.0)}, S, T)
    return res


# GradualGainerRetest.signal()'s per-candle outcome, as uint8 codes
# (bq_retest_replay's BQ_RT_*), and the detail bits beside them
(RT_IDLE, RT_WATCH_SET, RT_WATCHING, RT_RISK_BLOCKED, RT_CANDIDATE, RT_SHORT_HISTORY) = range(6)
RT_NO_FRAME = _lib.BQ_RT_NO_FRAME   # t < from_t[s] or t >= lens[s]: no message replayed
RT_EVENTS = dict(enumerate(_lib.RT_EVENTS))
RT_D_SUPPORT, RT_D_PULLBACK, RT_D_RECLAIM, RT_D_EXPIRED = (_lib.BQ_RT_D_SUPPORT, _lib.BQ_RT_D_PULLBACK,
                                                          _lib.BQ_RT_D_RECLAIM, _lib.BQ_RT_D_EXPIRED)


class RetestState:
    """The watchlist of GradualGainerRetest for S rows (its strategy_states
    entries): active uint8, started int64 (ms; expires_at = started +
    watch_ms), level float64 (the breakout level), each [S] on the device.
    signals.gradual_gainer_retest / engine.retest_replay update it in place,
    so a captured graph carries it from one replay to the next."""

    __slots__ = ("active", "started", "level")

    def __init__(self, active: torch.Tensor, started: torch.Tensor, level: torch.Tensor):
        self.active, self.started, self.level = active, started, level

    @classmethod
    def idle(cls, S: int, device) -> "RetestState":
        return cls(torch.zeros(S, dtype=torch.uint8, device=device), torch.zeros(S, dtype=torch.int64, device=device),
                   torch.full((S,), NAN, dtype=torch.float64, device=device))

    def tensors(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.active, self.started, self.level


def gradual_gainer_retest(o, h, l, c, open_time, btc_time, btc_close, *, risk_ok=None, state: RetestState | None = None,
                          first_t=None, lens=None, from_t=None, leadership=None, ema20=None, **params):
    """The body of GradualGainerRetest.signal() (strategies/gradual_gainer_retest.py
    :222-308) for every candle of the panel: the leadership (unless given:
    gradual_gainer_leadership's dict), the frame's EMA20 (unless given) and
    the watchlist replay (engine.retest_replay, bq_retest_replay). Column t of
    row s = the method on the message whose frame is df.iloc[first_t[s]:t + 1],
    after the messages of all earlier candles; candles from_t[s] ..
    lens[s] - 1 are replayed, from `state` (None: idle), which is updated in
    place. risk_ok [S, T] bool: _risk_allows per candle (retest_risk_allows;
    None: always allowed). open_time ascends strictly within a row's frame.

    The leadership and the EMA computed here are the whole row's: for rows
    with first_t > 0 pass `leadership` / `ema20` of the trimmed frame (or the
    trimmed row itself). params: engine.RETEST_DEFAULTS' keys.

    Returns {"event": uint8 [S, T] (RT_* codes, RT_EVENTS their names),
    "detail": uint8 [S, T] (RT_D_* bits: the failed tests of a watching
    candle; RT_D_EXPIRED where the watch expired on this candle),
    "breakout_level": [S, T] (the level in force at watch_set / watching /
    risk_blocked / candidate candles, NaN elsewhere), "leader", "rs_2h",
    "rs_6h", "ema20"}."""
    lead = leadership if leadership is not None else gradual_gainer_leadership(open_time, c, btc_time, btc_close)
    e20 = ema20 if ema20 is not None else ema(c, 20)
    event, detail, level = engine.retest_replay(o, h, l, c, e20, open_time, lead["leader"], risk_ok,
                                                state=state.tensors() if state is not None else None,
                                                first_t=first_t, lens=lens, from_t=from_t, **params)
    return {"event": event, "detail": detail, "breakout_level": level, "leader": lead["leader"],
            "rs_2h": lead["rs_2h"], "rs_6h": lead["rs_6h"], "ema20": e20}


# GradualGainerRetest._risk_allows' reasons (:198-215), as uint8 codes: the first failing check in the method's order
RISK_REASONS = ("risk_profile_allows_long", "market_context_unavailable", "market_stress_too_high", "btc_context_down",
                "symbol_regime_unavailable", "symbol_atr_too_high", "symbol_transition_not_long", "symbol_trend_down")


def retest_risk_allows(market_stress_score, btc_regime_score, btc_return, context_ok, atr_pct, micro_regime,
                       micro_transition, trend_score, features_ok, max_market_stress: float = 0.25,
                       max_atr_pct: float = 0.06):
    """GradualGainerRetest._risk_allows (strategies/gradual_gainer_retest.py:198-215)
    per (symbol, candle): the context's market_stress_score / btc_regime_score
    / btc_return [T] float64 and context_ok [T] bool (False: no context), the
    symbol features atr_pct / trend_score [S, T] float64, micro_regime /
    micro_transition [S, T] int8 (_lib.MICRO_REGIMES / MICRO_TRANSITIONS
    codes, negative: none) and features_ok [S, T] bool (False: the context
    has no features for the symbol). Returns (ok bool [S, T], reason uint8
    [S, T]): the first failing check in the method's order, RISK_REASONS its
    strings (0 = risk_profile_allows_long). One fused element-wise program."""
    S, T = atr_pct.shape
    down, breakdown, entered_down = (float(_lib.MICRO_REGIMES.index("TREND_DOWN")),
                                     float(_lib.MICRO_TRANSITIONS.index("BREAKDOWN")),
                                     float(_lib.MICRO_TRANSITIONS.index("ENTERED_TREND_DOWN")))
    STRESS, REG, RET = F.inp(market_stress_score), F.inp(btc_regime_score), F.inp(btc_return)
    ATR, TREND = F.inp(atr_pct), F.inp(trend_score)
    MR, MT = F.inp(micro_regime.to(torch.float64)), F.inp(micro_transition.to(torch.float64))
    checks = [~F.inp(context_ok), STRESS >= max_market_stress, (REG < -0.2) & (RET < 0.0), ~F.inp(features_ok),
              ATR > max_atr_pct, (MT == breakdown) | (MT == entered_down), (MR == down) & (TREND < 0.0)]
    code = F.const(0.0)
    for i in range(len(checks), 0, -1):
        code = F.where(checks[i - 1], float(i), code)
    reason = F.run({"reason": code}, S, T)["reason"].to(torch.uint8)
    return reason == 0, reason


# FailedSpikeFade.signal()'s per-candle outcome, as uint8 codes
# (bq_spike_fade_replay's BQ_FS_*), and the detail bits beside them
(FS_IDLE, FS_SOURCE_SET, FS_WAITING, FS_CANDIDATE, FS_CLEARED, FS_SAME_CANDLE) = range(6)
FS_NO_FRAME = _lib.BQ_FS_NO_FRAME   # t < max(from_t[s], first_t[s]) or t >= lens[s]: no message replayed
FS_EVENTS = dict(enumerate(_lib.FS_EVENTS))
(FS_D_SOURCE, FS_D_MARKET, FS_D_NEW_HIGH, FS_D_CANDLE_EXPIRED, FS_D_WINDOW_EXPIRED, FS_D_EXTENSION) = (
    _lib.BQ_FS_D_SOURCE, _lib.BQ_FS_D_MARKET, _lib.BQ_FS_D_NEW_HIGH, _lib.BQ_FS_D_CANDLE_EXPIRED,
    _lib.BQ_FS_D_WINDOW_EXPIRED, _lib.BQ_FS_D_EXTENSION)


class SpikeFadeState:
    """The pending spikes of FailedSpikeFade for S rows (its strategy_states
    entries): active uint8, and the source candle's open_time int64 (ms), high
    and close float64, each [S] on the device (the entry's volume and
    quote_asset_volume only feed the message text: gather them at t - bars).
    signals.failed_spike_fade / engine.spike_fade_replay update it in place,
    so a captured graph carries it from one replay to the next."""

    __slots__ = ("active", "open_time", "high", "close")

    def __init__(self, active: torch.Tensor, open_time: torch.Tensor, high: torch.Tensor, close: torch.Tensor):
        self.active, self.open_time, self.high, self.close = active, open_time, high, close

    @classmethod
    def idle(cls, S: int, device) -> "SpikeFadeState":
        return cls(torch.zeros(S, dtype=torch.uint8, device=device), torch.zeros(S, dtype=torch.int64, device=device),
                   torch.full((S,), NAN, dtype=torch.float64, device=device),
                   torch.full((S,), NAN, dtype=torch.float64, device=device))

    def tensors(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.active, self.open_time, self.high, self.close


# FailedSpikeFade.source_spike_allows' strings (:190-203), as uint8 codes: 0 allows, then the first failing check
SPIKE_SOURCE_REASONS = ("symbol_confirmed_upward_price_impulse", "symbol_price_impulse_missing",
                        "symbol_spike_too_extended", "symbol_upward_spike_missing")
# source_market_allows / failure_market_allows' strings (:155-188): 0 and 1 allow (the reference appends the
# breadth series' key, "_market_breadth_ma" or "_market_breadth", to them), then the first failing check
SPIKE_MARKET_REASONS = ("source_breadth_up", "failure_breadth_down", "market_context_unavailable",
                        "market_stress_too_high", "market_context_not_long", "breadth_momentum_unavailable",
                        "source_breadth_not_up", "failure_breadth_not_down")


def _first_true(checks, none: float):
    """The code beside the first true check (`none` when none is)."""
    code = F.const(none)
    for cond, value in reversed(checks):
        code = F.where(cond, float(value), code)
    return code


def spike_source_allows(label, price_break_flag, cumulative_price_break_flag, accel_spike_flag, close_open_ratio,
                        upward, max_candle_return: float = 0.06):
    """FailedSpikeFade.source_spike_allows (strategies/failed_spike_fade.py:190-203)
    per (symbol, candle) on failed_spike_features' columns: label, the three
    price-impulse flags and upward bool [S, T], close_open_ratio float64
    [S, T]. Returns (ok bool [S, T], reason uint8 [S, T]): the first failing
    check in the method's order, SPIKE_SOURCE_REASONS its strings (0 = allowed).
    A NaN close_open_ratio passes, as nan > x does. One fused element-wise
    program."""
    S, T = close_open_ratio.shape
    impulse = F.inp(price_break_flag) | F.inp(cumulative_price_break_flag) | F.inp(accel_spike_flag)
    code = _first_true([(~F.inp(label) | ~impulse, 1), (F.inp(close_open_ratio) > max_candle_return, 2),
                        (~F.inp(upward), 3)], 0.0)
    reason = F.run({"reason": code}, S, T)["reason"].to(torch.uint8)
    return reason == 0, reason


def spike_source_frames(o, h, l, c, v, qv, p=None, *, first_t=None, lens=None, from_t=None, exact: bool = True,
                        max_candle_return: float = 0.06, frame_cap: int | None = None):
    """FailedSpikeFade.source_spike_allows on the message of EVERY candle:
    spike_source_allows over strategies.failed_spike_frames' columns, column t
    of row s from latest_signal() of a fresh instance on the frame
    df.iloc[first_t[s]:t + 1]. Returns (ok bool [S, T], reason uint8 [S, T]),
    ok ready for failed_spike_fade(source_ok=...); outside the formed candles
    ok is False (reason 1: no label there). p: strategies.SpikeParams; the
    other arguments are failed_spike_frames', frame_cap among them (the live
    store's sliding frame: df.iloc[max(first_t[s], t + 1 - frame_cap):t + 1])."""
    from . import strategies

    f = strategies.failed_spike_frames(o, h, l, c, v, qv, p, first_t=first_t, lens=lens, from_t=from_t, exact=exact,
                                       frame_cap=frame_cap,
                                       columns=("label", "price_break_flag", "cumulative_price_break_flag",
                                                "accel_spike_flag", "close_open_ratio", "upward"))
    return spike_source_allows(f["label"], f["price_break_flag"], f["cumulative_price_break_flag"],
                               f["accel_spike_flag"], f["close_open_ratio"], f["upward"], max_candle_return)


def spike_fade_market_allows(market_stress_score, long_regime_score, short_regime_score, context_ok, momentum_points,
                             max_market_stress: float = 0.35, min_momentum: float = 0.5):
    """FailedSpikeFade.source_market_allows / failure_market_allows
    (strategies/failed_spike_fade.py:155-188) per candle: the context's
    market_stress_score / long_regime_score / short_regime_score [T] float64,
    context_ok [T] bool (False: no context) and momentum_points [T] float64,
    the caller's _breadth_momentum_points (NaN: breadth_momentum_unavailable).
    Returns (source_ok bool, source_reason uint8, failure_ok bool,
    failure_reason uint8), each [T]; the reasons index SPIKE_MARKET_REASONS
    (0 / 1: the source / the failure gate allows). One fused element-wise
    program."""
    T = momentum_points.numel()
    STRESS, LONG, SHORT, MOM = (F.inp(x.reshape(-1)) for x in (market_stress_score, long_regime_score,
                                                              short_regime_score, momentum_points))
    head = [(~F.inp(context_ok.reshape(-1)), 2), (STRESS >= max_market_stress, 3)]
    src = _first_true(head + [(LONG <= SHORT, 4), (F.isnan(MOM), 5), (~(MOM >= min_momentum), 6)], 0.0)
    fail = _first_true(head + [(F.isnan(MOM), 5), (~(MOM <= -min_momentum), 7)], 1.0)
    res = F.run({"src": src, "fail": fail}, 1, T)
    src_reason, fail_reason = res["src"].reshape(-1).to(torch.uint8), res["fail"].reshape(-1).to(torch.uint8)
    return src_reason == 0, src_reason, fail_reason == 1, fail_reason


def failed_spike_fade(o, h, c, open_time, source_ok, *, src_market=None, fail_market=None,
                      state: SpikeFadeState | None = None, first_t=None, lens=None, from_t=None, **params):
    """The body of FailedSpikeFade.signal() (strategies/failed_spike_fade.py
    :596-695) for every candle of the panel: the pending-spike replay
    (engine.spike_fade_replay, bq_spike_fade_replay). Column t of row s = the
    method on the message whose frame is df.iloc[first_t[s]:t + 1], after the
    messages of all earlier candles; candles from_t[s] .. lens[s] - 1 are
    replayed, from `state` (None: idle), which is updated in place. open_time
    ascends strictly within a row's frame.

    source_ok [S, T] bool: column t must hold source_spike_allows of the
    FRAME ENDING AT t (spike_source_allows on the newest column of
    strategies.failed_spike_features of that frame). The cohort's newest
    column is exactly that, and spike_source_frames forms it for every
    candle of a panel in about one pass (strategies.failed_spike_frames: the
    per-prefix detect()). A whole-row failed_spike_features over a long panel
    is NOT it: detect()'s auto-calibration and cooldown are frame-wide, so an
    earlier column of a long frame is not what the message at that candle
    saw. src_market / fail_market:
    spike_fade_market_allows' source_ok / failure_ok, bool [T] or [S, T]
    (None: allowed). params: engine.SPIKE_FADE_DEFAULTS' keys.

    Returns {"event": uint8 [S, T] (FS_* codes, FS_EVENTS their names),
    "detail": uint8 [S, T] (FS_D_* bits: the gate(s) that kept an idle candle
    idle, the failed test(s) of a waiting candle, the reason a spike was
    cleared), "bars": uint8 [S, T] (bars_elapsed at waiting / candidate /
    cleared-by-window-or-extension candles, 0 elsewhere)}."""
    event, detail, bars = engine.spike_fade_replay(o, h, c, open_time, source_ok, src_market, fail_market,
                                                   state=state.tensors() if state is not None else None,
                                                   first_t=first_t, lens=lens, from_t=from_t, **params)
    return {"event": event, "detail": detail, "bars": bars}


# RelativeStrengthImpulseRider._features reason strings, as uint8 codes
# (the first failing check in the method's order; bq_impulse_rider's BQ_IR_*)
(IR_CONFIRMED, IR_SHORT_HISTORY, IR_INVALID_VALUES, IR_INVALID_ANCHORS, IR_BTC_UNAVAILABLE, IR_RANGE_INVALID,
 IR_NOT_READY, IR_IMPULSE_RANGE, IR_DID_NOT_CROSS, IR_BTC_TOO_HIGH, IR_RS_TOO_LOW, IR_ATR_TOO_HIGH, IR_DID_NOT_HOLD,
 IR_CONFIRMATION_NEGATIVE, IR_CLOSE_NOT_NEAR_HIGH) = range(15)
IR_NO_FRAME = _lib.BQ_IR_NO_FRAME   # t >= lens[s]: no such prefix frame (not a reference reason)
IR_REASONS = {
    IR_CONFIRMED: "relative_strength_impulse_confirmed",
    IR_SHORT_HISTORY: "history_too_short",
    IR_INVALID_VALUES: "invalid_candle_values",
    IR_INVALID_ANCHORS: "invalid_return_anchors",
    IR_BTC_UNAVAILABLE: "btc_return_unavailable",
    IR_RANGE_INVALID: "confirmation_range_invalid",
    IR_NOT_READY: "indicators_not_ready",
    IR_IMPULSE_RANGE: "impulse_outside_range",
    IR_DID_NOT_CROSS: "impulse_did_not_cross_threshold",
    IR_BTC_TOO_HIGH: "btc_return_too_high",
    IR_RS_TOO_LOW: "relative_strength_too_low",
    IR_ATR_TOO_HIGH: "atr_pct_too_high",
    IR_DID_NOT_HOLD: "confirmation_did_not_hold_trigger_close",
    IR_CONFIRMATION_NEGATIVE: "confirmation_return_negative",
    IR_CLOSE_NOT_NEAR_HIGH: "confirmation_close_not_near_high",
}
IR_KEYS = _lib.IMPULSE_VALUES


def impulse_rider_features(o, h, l, c, atr, open_time, btc_time, btc_close, *, first_t=None, lens=None,
                           columns=IR_KEYS, check_bench: bool = True, **thresholds):
    """RelativeStrengthImpulseRider._features evaluated at every t
    (strategies/relative_strength_impulse_rider.py:92-198): column t = the
    method on the prefix frame df.iloc[first_t[s]:t + 1] (first_t: the rows
    Candles.post_process dropped, default 0) against the benchmark frame
    (btc_time ascending, a repeated time resolves to its last row, as
    _btc_return_at's backwards scan does, :74-81). atr is the frame's ATR
    column (e.g. engine.enrich(...)["ATR"]). One pass (engine.impulse_rider,
    bq_impulse_rider).

    Returns (values, status): values maps IR_KEYS (or the requested subset)
    to [S, T] float64 — bit for bit the method's value where status ==
    IR_CONFIRMED, NaN elsewhere (the method returns None there) — and status
    is [S, T] uint8: the first failing check (IR_* codes, IR_REASONS gives the
    reference's reason string), IR_NO_FRAME where t >= lens[s]. trigger_close,
    confirmation_close and the two open times of the method's dict are the
    caller's own close[t - 1], close[t], open_time[t - 1], open_time[t].
    thresholds: min_history, min_impulse, max_impulse, min_rs, max_btc_return,
    min_conf_return, min_close_location, max_atr_pct, entry_factor
    (1 - RETEST_DISCOUNT_PCT / 100, formed in Python floats)."""
    return engine.impulse_rider(o, h, l, c, atr, open_time, btc_time, btc_close, first_t=first_t, lens=lens,
                                columns=columns, check_bench=check_bench, **thresholds)


# TopGainerEarlyMomentum's decisions, as uint8 codes (bq_top_gainer_entry's
# BQ_TGE_*): the feature status, the first failing check of _entry_allows, the
# two confirmation rules and the risk branch. Code 0 reads
# top_gainer_breakout_ignition in the `entry` column (TGE_ENTRY_REASONS) and
# top_gainer_breakout_two_close_confirmation in `status` (TGE_REASONS).
(TGE_CONFIRMED, TGE_SHORT_HISTORY, TGE_INVALID_CANDLE, TGE_NOT_READY, TGE_NOT_BREAKING, TGE_NOT_ABOVE_EMAS,
 TGE_NOT_GREEN, TGE_CANDLE_EXTENDED, TGE_HOUR_EXTENDED, TGE_EXTENSION, TGE_NOT_ACCELERATING, TGE_SIX_HOUR,
 TGE_VOLUME_LOW, TGE_NOT_NEAR_HIGH, TGE_UPPER_WICK, TGE_FIRST_CONFIRM, TGE_SECOND_CONFIRM,
 TGE_RISK_REJECTED) = range(18)
TGE_NO_FRAME = _lib.TGE_NO_FRAME   # t >= lens[s]: no such message (not a reference reason)
TGE_REASONS = dict(enumerate(_lib.TGE_REASONS))
TGE_ENTRY_REASONS = {**{k: v for k, v in TGE_REASONS.items() if k < TGE_FIRST_CONFIRM},
                     TGE_CONFIRMED: _lib.TGE_ENTRY_OK}
TGE_KEYS = _lib.TGE_VALUES


def top_gainer_entry(o, h, l, c, v, qv=None, atr=None, *, risk_ok=None, first_t=None, lens=None, columns=TGE_KEYS,
                     **thresholds):
    """TopGainerEarlyMomentum.signal() up to the message (strategies/
    top_gainer_early_momentum.py:363-406) for every candle of the panel, with
    its _features (:91-159) and _entry_allows (:161-188), in one pass
    (engine.top_gainer_entry, bq_top_gainer_entry). Column t of row s = the
    reference on the frame df.iloc[first_t[s]:t + 1] (first_t: the rows
    Candles.post_process dropped, default 0). qv: the quote_asset_volume
    column (None: the reference's volume * close fall-backs); atr: the frame's
    ATR column (None: 0.0); risk_ok [S, T] bool: _risk_profile_allows per
    candle (top_gainer_risk_allows; None: allowed).

    Returns {"status": uint8 [S, T], signal()'s outcome for the message whose
    newest candle is t (TGE_* codes, TGE_REASONS their strings; 0 =
    top_gainer_breakout_two_close_confirmation, TGE_NO_FRAME where
    t >= lens[s]); "entry": uint8 [S, T], the feature status or the first
    failing check of _entry_allows on the prefix frame ending at t
    (TGE_ENTRY_REASONS; 0 = top_gainer_breakout_ignition); "score" /
    "stop_loss_pct": [S, T] float64, _score of the breakout candle t - 2 and
    _stop_loss_pct(close[t], atr[t]) where status is 0 or TGE_RISK_REJECTED,
    NaN elsewhere — both UNROUNDED: the reference's round_numbers(.., 4) is
    pybinbot's and stays a host step; "values": {key: [S, T] float64} for
    `columns` (a subset of TGE_KEYS), the prefix frame's value where the
    feature status is ready, NaN elsewhere (top_gainer_features' convention)}.
    The point-wise values are the reference's bits; ema20 / ema50 and the two
    volume ratios agree with pandas to rounding. _already_emitted compares
    open times for equality only and stays with the host. thresholds:
    engine.TOP_GAINER_DEFAULTS' keys."""
    status, entry, score, stop, values = engine.top_gainer_entry(o, h, l, c, v, qv, atr, risk_ok=risk_ok,
                                                                 first_t=first_t, lens=lens, columns=columns,
                                                                 **thresholds)
    return {"status": status, "entry": entry, "score": score, "stop_loss_pct": stop, "values": values}


# TopGainerEarlyMomentum._risk_profile_allows' reasons (:204-234), as uint8 codes: the first failing check in the
# method's order
TG_RISK_REASONS = ("risk_profile_allows_long", "market_context_unavailable", "market_stress_too_high",
                   "market_context_short_edge", "btc_context_down", "symbol_regime_unavailable",
                   "relative_strength_vs_btc_not_positive", "symbol_atr_too_high", "symbol_transition_not_long",
                   "symbol_trend_down")


def top_gainer_risk_allows(market_stress_score, long_regime_score, short_regime_score, btc_regime_score, btc_return,
                           context_ok, relative_strength_vs_btc, atr_pct, micro_regime, micro_transition,
                           trend_score, features_ok, max_market_stress: float = 0.25,
                           min_relative_strength: float = 0.03, max_atr_pct: float = 0.06):
    """TopGainerEarlyMomentum._risk_profile_allows (strategies/top_gainer_early_momentum.py
    :204-234) per (symbol, candle): the context's market_stress_score /
    long_regime_score / short_regime_score / btc_regime_score / btc_return [T]
    float64 and context_ok [T] bool (False: no context), the symbol features
    relative_strength_vs_btc / atr_pct / trend_score [S, T] float64,
    micro_regime / micro_transition [S, T] int8 (_lib.MICRO_REGIMES /
    MICRO_TRANSITIONS codes, negative: none) and features_ok [S, T] bool
    (False: the context has no features for the symbol). Returns (ok bool
    [S, T], reason uint8 [S, T]): the first failing check in the method's
    order, TG_RISK_REASONS its strings (0 = risk_profile_allows_long). One
    fused element-wise program."""
    S, T = atr_pct.shape
    down = float(_lib.MICRO_REGIMES.index("TREND_DOWN"))
    blocked = [float(_lib.MICRO_TRANSITIONS.index(k)) for k in ("BREAKDOWN", "ENTERED_TREND_DOWN",
                                                                "VOLATILITY_EXPANSION")]
    STRESS, LONG, SHORT = F.inp(market_stress_score), F.inp(long_regime_score), F.inp(short_regime_score)
    REG, RET = F.inp(btc_regime_score), F.inp(btc_return)
    RS, ATR, TREND = F.inp(relative_strength_vs_btc), F.inp(atr_pct), F.inp(trend_score)
    MR, MT = F.inp(micro_regime.to(torch.float64)), F.inp(micro_transition.to(torch.float64))
    checks = [~F.inp(context_ok), STRESS >= max_market_stress, SHORT > LONG + 0.15, (REG < -0.2) & (RET < 0.0),
              ~F.inp(features_ok), RS <= min_relative_strength, ATR > max_atr_pct,
              (MT == blocked[0]) | (MT == blocked[1]) | (MT == blocked[2]), (MR == down) & (TREND < 0.0)]
    code = F.const(0.0)
    for i in range(len(checks), 0, -1):
        code = F.where(checks[i - 1], float(i), code)
    reason = F.run({"reason": code}, S, T)["reason"].to(torch.uint8)
    return reason == 0, reason


# ---- LiquidationSweepPump: the candidate gate and the cohort winner -----------------------------------------------
# bq_sweep_select's status codes: the first failing check of signal() in the method's order (:314, :287-299, :331,
# :343); SW_REASONS names them (the reference returns silently, so the names are this library's)
(SW_CANDIDATE, SW_SHORT_FRAME, SW_NOT_FINITE, SW_NO_CROSS, SW_MOMENTUM_ATR, SW_NOT_ABOVE_PRIOR_HIGH,
 SW_CLOSE_LOCATION, SW_VOLUME, SW_TREND, SW_BELOW_EMA20, SW_RELATIVE_STRENGTH, SW_BTC_MOMENTUM, SW_BTC_TREND,
 SW_THRESHOLD_NONPOSITIVE, SW_ROUTE_REFUSED) = range(15)
SW_NO_FRAME = _lib.SW_NO_FRAME   # u + 1 >= lens[s] or u < first_t[s]: no such message (not a reference outcome)
SW_REASONS = dict(enumerate(_lib.SW_REASONS))
SW_COLUMNS = _lib.SW_COLUMNS     # the 13 values _is_candidate requires, in its order; plus "score_cross"


def liquidation_sweep_select(cols, *, close=None, route_ok=None, first_t=None, lens=None, symbol_rank=None,
                             t_range=None, params=None):
    """LiquidationSweepPump.signal() between compute_pump_score and the
    portfolio selector (strategies/liquidation_sweep_pump.py:302-343), and the
    selector's pick per candle time (:78-81), for every trigger candle of the
    panel in one call (engine.sweep_select, bq_sweep_select).

    cols: the dict strategies.pump_score_features returns, or any mapping with
    SW_COLUMNS' 13 keys and "score_cross" ([S, T]); pump_score_features does
    not return the frame's own close, so it is taken from cols["close"] or
    from `close=`. Column u is the TRIGGER candle — the decision signal()
    takes on df.iloc[-2] at the message whose frame is df.iloc[first_t[s] :
    u + 2]; the rows share one open-time grid, so a column is one cohort of
    the selector. route_ok [S, T] bool: long_entry_routing's verdict per cell
    (sweep_routing_allows; None: allowed). symbol_rank [S] int32 on the
    device: each row's position in the str order of the symbol names — the
    selector's tie-break is max(key=(rank_score, symbol)) (None: the row
    index). t_range (t_lo, t_hi): decide these columns only; the others'
    outputs are not written (uninitialised). params: engine.SWEEP_DEFAULTS'
    keys.

    Returns {"status": uint8 [S, T] (SW_* codes, SW_REASONS their names; 0 =
    the candidate signal() submits; SW_NO_FRAME where there is no such
    message), "candidate": bool [S, T] (status == 0), "rank_score": float64
    [S, T], pump_score / score_threshold where status == 0 and NaN elsewhere,
    "winner": int64 [T], the row _dispatch_winner dispatches for that candle
    time or -1, "winner_score": float64 [T], its rank_score or NaN}. Status,
    rank_score and the winner are exact given the columns. What stays on the
    host: the message text, observe() / the cohorts' bookkeeping and the
    dispatch."""
    missing = [k for k in SW_COLUMNS + ("score_cross",) if k not in cols and not (k == "close" and close is not None)]
    if missing:
        raise ValueError(f"liquidation_sweep_select: missing columns {missing}")
    cs = [close if k == "close" and close is not None else cols[k] for k in SW_COLUMNS]
    status, rank, winner, wscore = engine.sweep_select(cs, cols["score_cross"], route_ok=route_ok, first_t=first_t,
                                                       lens=lens, symbol_rank=symbol_rank, t_range=t_range,
                                                       **(params or {}))
    return {"status": status, "candidate": status == 0, "rank_score": rank, "winner": winner,
            "winner_score": wscore}


# LiquidationSweepPump.long_entry_routing's reasons (:164-193) as uint8 codes: the refusals in the method's order,
# then the accepting route
SW_ROUTE_REASONS = ("market_context_unavailable", "market_stress_too_high", "market_breadth_not_washed_out",
                    "market_breadth_not_recovering", "btc_not_increasing", "symbol_regime_unavailable",
                    "symbol_trend_not_up", "market_breadth_recovering_btc_up_symbol_up")
SW_ROUTE_OK = len(SW_ROUTE_REASONS) - 1


def sweep_routing_allows(market_stress_score, market_breadth, market_breadth_recovery, context_ok, btc_momentum,
                         symbol_trend_score, features_ok, max_market_stress: float = 0.35,
                         breadth_threshold: float = -0.2, min_breadth_recovery: float = 0.02):
    """LiquidationSweepPump.long_entry_routing (strategies/liquidation_sweep_pump.py
    :164-193) per (symbol, candle): the context's market_stress_score, the
    latest market breadth and its recovery values[-1] - values[-3] ([T] or
    [S, T] float64; a NaN recovery is the method's None: fewer than three
    breadth values) and context_ok bool (False: no context); btc_momentum
    [S, T] float64 (the trigger row's btc_momentum_3), symbol_trend_score
    [S, T] float64 and features_ok [S, T] bool (False: the context has no
    features for the symbol). Returns (ok bool [S, T], reason uint8 [S, T]):
    the first refusing check in the method's order, SW_ROUTE_REASONS its
    strings (SW_ROUTE_OK = the accepting route). One fused element-wise
    program. _market_breadth_values' timestamp parsing and sorting of the API
    series (:135-153) is a host step: the caller passes the sorted series'
    last value and recovery, or the context's advancers - decliners."""
    S, T = symbol_trend_score.shape
    STRESS, BREADTH, REC = F.inp(market_stress_score), F.inp(market_breadth), F.inp(market_breadth_recovery)
    BTC, TREND = F.inp(btc_momentum), F.inp(symbol_trend_score)
    code = _first_true([(~F.inp(context_ok), 0), (STRESS >= max_market_stress, 1), (BREADTH > breadth_threshold, 2),
                        (F.isnan(REC) | (REC < min_breadth_recovery), 3), (BTC <= 0.0, 4),
                        (~F.inp(features_ok), 5), (TREND <= 0.0, 6)], float(SW_ROUTE_OK))
    reason = F.run({"reason": code}, S, T)["reason"].to(torch.uint8)
    return reason == SW_ROUTE_OK, reason


def bb_width_stable(bb_upper, bb_mid, bb_lower, n: int = 8, max_change_pct: float = 20.0, *, first_t=None,
                    lens=None) -> dict[str, torch.Tensor]:
    """LadderDeployer._bb_stable(n, max_change_pct) evaluated at every t
    (strategies/grid/ladder_deployer.py:42-56; the strategy calls it with
    MIN_BB_WIDTH_STABILITY_CANDLES = 8, MAX_BB_WIDTH_CHANGE_PCT = 20.0) on the
    prefix frame df.iloc[first_t[s]:t + 1]. Returns {"stable": bool [S, T],
    "change_pct": float64 [S, T]}: change_pct is abs((w[-1] - w[0]) / w[0]) *
    100 over the last n widths (upper - lower) / mid where the method reaches
    it, NaN where it returns earlier (fewer than n rows, a row with mid <= 0
    or width <= 0). One pass (engine.bb_stable, bq_bb_stable)."""
    stable, change = engine.bb_stable(bb_upper, bb_mid, bb_lower, n, max_change_pct, first_t=first_t, lens=lens)
    return {"stable": stable, "change_pct": change}


def mean_reversion_features(o, h, l, c, v, atr, rsi_window: int = 14, volume_ma_window: int = 20,
                            atr_ma_window: int = 20, fast: int = 20, slow: int = 50) -> dict[str, torch.Tensor]:
    """The per-candle inputs MeanReversionFade reads (strategies/mean_reversion_fade.py:240-255):
    rsi / previous_rsi, volume_ma, atr_ma, trend_score and the upper rejection
    ratio of _resolve_entry (:124-134)."""
    rsi = _rsi_ex(c, rsi_window)
    vma, ama = engine.rolling_many(engine.Roll(v, volume_ma_window, "mean"), engine.Roll(atr, atr_ma_window, "mean"))
    H, L, O, C = F.inp(h), F.inp(l), F.inp(o), F.inp(c)
    rng = H - L
    res = F.run({
        "rsi": rsi,
        "previous_rsi": F.shift(rsi, 1),
        "trend_score": _trend_ex(c, fast, slow),
        "upper_rejection_ratio": F.where(rng > 0, (H - F.maximum(O, C)) / rng, NAN),
    })
    return {"rsi": res["rsi"], "previous_rsi": res["previous_rsi"], "volume_ma": vma, "atr_ma": ama,
            "trend_score": res["trend_score"], "upper_rejection_ratio": res["upper_rejection_ratio"]}


# bq_mean_reversion_replay's status codes: where MeanReversionFade.signal() returned, in the method's order
# (MR_REASONS: the method's own log reasons; "emit" and "no_frame" are this library's)
MR_EMIT, MR_NO_FRAME, MR_NOT_READY = range(3)
MR_REASONS = dict(enumerate(_lib.MR_REASONS))
MR_VALUES = _lib.MR_VALUES
MR_FEATURES = _lib.MR_VALUES[:_lib.MR_NFEATURES]
MR_CTX_ROWS = _lib.MR_CTX_ROWS
MR_SYM_KEYS = ("ok", "atr_pct", "trend_score", "micro_regime", "micro_transition")


class MeanReversionState:
    """MeanReversionFade's entries of strategy_cooldowns for S rows: has uint8
    (the (ALGO, symbol) key is present) and last_open_time int64 (the open
    time of the last emitted candle), each [S] on the device.
    signals.mean_reversion_fade_entry / engine.mean_reversion_replay update it
    in place, so a captured graph carries it from one message to the next."""

    __slots__ = ("has", "last_open_time")

    def __init__(self, has: torch.Tensor, last_open_time: torch.Tensor):
        self.has, self.last_open_time = has, last_open_time

    @classmethod
    def empty(cls, S: int, device) -> "MeanReversionState":
        return cls(torch.zeros(S, dtype=torch.uint8, device=device), torch.zeros(S, dtype=torch.int64, device=device))

    def clone(self) -> "MeanReversionState":
        return MeanReversionState(self.has.clone(), self.last_open_time.clone())

    def tensors(self) -> tuple[torch.Tensor, torch.Tensor]:
        return self.has, self.last_open_time


def _pick(d, keys, what: str):
    """A {name: tensor} argument (`what`: "sym" / "features") as the tuple in `keys` order; None stays None."""
    if d is None:
        return None
    missing = [k for k in keys if k not in d]
    if missing:
        raise ValueError(f"{what}: missing {missing} (expected {keys})")
    return tuple(d[k] for k in keys)


def mean_reversion_fade_entry(o, h, l, c, v, atr, bb_upper, open_time, ctx, ctx_ok=None, *, sym=None, features=None,
                              state: MeanReversionState | None = None, first_t=None, lens=None, from_t=None,
                              columns=MR_VALUES, **params):
    """The decisions of MeanReversionFade.signal() (strategies/mean_reversion_fade.py
    :224-300) for every candle of a 15m panel in one pass
    (engine.mean_reversion_replay, bq_mean_reversion_replay). Column t of row
    s = the method on the message whose frame is df_15m.iloc[first_t[s]:t + 1],
    after the messages of all earlier candles; candles from_t[s] .. lens[s] - 1
    are replayed, from `state` (None: no candle emitted yet), which is updated
    in place. o / h / l / c / v / atr / bb_upper [S, T] float64 (the enriched
    frame's columns; bb_upper as the caller rounds it), open_time [S, T] int64
    ms. ctx [5, 1] or [5, T] float64 (MR_CTX_ROWS) and ctx_ok [1] / [T]
    (False: latest_market_context is None), both on the device. sym: None (no
    symbol has features in the snapshot) or {MR_SYM_KEYS: tensor}, all [S] or
    all [S, T]: ok (False: resolve_symbol_features gave None), atr_pct,
    trend_score, micro_regime / micro_transition as uint8 indices into
    _lib.MICRO_REGIMES / _lib.MICRO_TRANSITIONS (_lib.MR_NONE: None).
    features: None to form rsi, previous_rsi, volume_ma, atr_ma and
    trend_score in the pass (1e-9 of pandas), or mean_reversion_features'
    dictionary. params: engine.MEAN_REVERSION_DEFAULTS' keys.

    Returns {"status": uint8 [S, T] (MR_REASONS; 0 = the message goes out and
    the row's state moves to open_time[t]), and the `columns` of MR_VALUES,
    float64 [S, T], NaN where the method did not reach them}. stop_loss_pct
    and score are unrounded: round_numbers(.., 4) / round(.., 4), the FUTURES
    and ATR-column checks, the message text and the dispatch stay host
    steps."""
    sym, features = _pick(sym, MR_SYM_KEYS, "sym"), _pick(features, MR_FEATURES, "features")
    status, vals = engine.mean_reversion_replay(
        o, h, l, c, v, atr, bb_upper, open_time, ctx, ctx_ok, sym=sym, features=features,
        state=state.tensors() if state is not None else None, first_t=first_t, lens=lens, from_t=from_t,
        columns=columns, **params)
    return {"status": status, **vals}


# bq_range_fade_replay's status codes: where RangeBbRsiMeanReversion.signal() returned, in the method's order
# (RF_REASONS: regime_routing's reasons by their fixed part; "emit", "no_frame", "not_enough_data" and
# "adx_too_high" are this library's names for returns the method does not name)
(RF_EMIT, RF_NO_FRAME, RF_NOT_ENOUGH_DATA, RF_NO_CONTEXT, RF_TRANSITIONING, RF_STRESS, RF_NO_REGIME,
 RF_REGIME_NOT_RANGE, RF_NO_SYMBOL, RF_SYMBOL_NOT_RANGE, RF_SYMBOL_TRANSITION, RF_SYMBOL_ATR, RF_SYMBOL_BB_WIDTH,
 RF_ADX_TOO_HIGH, RF_NO_SETUP) = range(15)
RF_REASONS = dict(enumerate(_lib.RF_REASONS))
RF_VALUES = _lib.RF_VALUES
RF_FEATURES = _lib.RF_VALUES[:_lib.RF_NFEATURES]
RF_CTX_ROWS = _lib.RF_CTX_ROWS
RF_SYM_KEYS = ("ok", "micro_regime", "micro_transition", "atr_pct", "bb_width")
RF_LONG, RF_SHORT = 0.0, 1.0   # the `direction` column (bq_direction)


def range_fade_entry(o, h, l, c, v, rsi, bb_upper, bb_mid, bb_lower, ctx, ctx_ok=None, *, sym=None, features=None,
                     first_t=None, lens=None, from_t=None, columns=RF_VALUES, **params):
    """The decisions of RangeBbRsiMeanReversion.signal()
    (strategies/range_bb_rsi_mean_reversion.py:202-274) for every candle of a
    15m panel in one pass (engine.range_fade_replay, bq_range_fade_replay):
    the frame and null gate, regime_routing, the ADX cut, the two band
    rejections with their RSI and z-score confirmation, and local_score.
    Column t of row s = the method on the message whose frame is
    df_15m.iloc[first_t[s]:t + 1]; candles from_t[s] .. lens[s] - 1 are
    replayed. o / h / l / c / v / rsi / bb_upper / bb_mid / bb_lower [S, T]
    float64 (the enriched frame's columns and the three bands as the caller
    rounds them; current_price is the close). ctx [3, 1] or [3, T] float64
    (RF_CTX_ROWS; market_regime an index into _lib.MARKET_REGIMES,
    _lib.MR_NONE for None) and ctx_ok [1] / [T] (False: latest_market_context
    is None), both on the device. sym: None (no symbol has features in the
    snapshot) or {RF_SYM_KEYS: tensor}, all [S] or all [S, T]: ok (False:
    resolve_symbol_features gave None), micro_regime / micro_transition as
    uint8 indices into _lib.MICRO_REGIMES / _lib.MICRO_TRANSITIONS
    (_lib.MR_NONE: None), atr_pct, bb_width. features: None to form adx and
    zscore in the pass over the frame starting at first_t (1e-9 of pandas), or
    {"adx", "zscore"} (e.g. signals.adx / signals.zscore, which answer on
    whole rows: first_t = 0 only). params: engine.RANGE_FADE_DEFAULTS' keys.

    Returns {"status": uint8 [S, T] (RF_REASONS; 0 = the message goes out),
    and the `columns` of RF_VALUES, float64 [S, T], NaN where the method did
    not reach them: adx from adx_too_high on, zscore from
    no_bb_rsi_rejection_setup on, direction (RF_LONG / RF_SHORT) and score
    (local_score, unrounded) where it emits}. The rounding of the bands, the
    message text and the dispatch stay host steps."""
    sym, features = _pick(sym, RF_SYM_KEYS, "sym"), _pick(features, RF_FEATURES, "features")
    status, vals = engine.range_fade_replay(
        o, h, l, c, v, rsi, bb_upper, bb_mid, bb_lower, ctx, ctx_ok, sym=sym, features=features, first_t=first_t,
        lens=lens, from_t=from_t, columns=columns, **params)
    return {"status": status, **vals}


# ---- the 5m strategies: PriceTracker and ActivityBurstPump --------------------------------------------------------
# bq_price_tracker_replay's status codes: where PriceTracker.signal() returned, in the method's order (the
# reference returns silently: PT_REASONS' names are this library's), and the rejection's detail bits
(PT_EMIT, PT_NO_FRAME, PT_NOT_READY, PT_NO_SETUP, PT_NO_CONTEXT, PT_CONTEXT_REJECTED, PT_COOLDOWN) = range(7)
PT_REASONS = dict(enumerate(_lib.PT_REASONS))
PT_D_FOLLOWTHROUGH, PT_D_RISK, PT_D_CONFIDENCE = (_lib.BQ_PT_D_FOLLOWTHROUGH, _lib.BQ_PT_D_RISK,
                                                  _lib.BQ_PT_D_CONFIDENCE)
PT_VALUES = _lib.PT_VALUES
PT_CTX_ROWS = _lib.PT_CTX_ROWS


class PriceTrackerState:
    """PriceTracker's entries of strategy_cooldowns for S rows: has uint8 (the
    (ALGO, symbol) key is present) and last_close_time int64 (ms), each [S] on
    the device. signals.price_tracker_entry / engine.price_tracker_replay
    update it in place, so a captured graph carries it from one message to
    the next."""

    __slots__ = ("has", "last_close_time")

    def __init__(self, has: torch.Tensor, last_close_time: torch.Tensor):
        self.has, self.last_close_time = has, last_close_time

    @classmethod
    def empty(cls, S: int, device) -> "PriceTrackerState":
        return cls(torch.zeros(S, dtype=torch.uint8, device=device), torch.zeros(S, dtype=torch.int64, device=device))

    def clone(self) -> "PriceTrackerState":
        return PriceTrackerState(self.has.clone(), self.last_close_time.clone())

    def tensors(self) -> tuple[torch.Tensor, torch.Tensor]:
        return self.has, self.last_close_time


def price_tracker_entry(c, rsi, macd, mfi, close_time, symbol_rs, ctx, ctx_ok=None, *, h=None, l=None, v=None,
                        trend_score=None, state: PriceTrackerState | None = None, first_t=None, lens=None,
                        from_t=None, columns=PT_VALUES, **params):
    """The decisions of PriceTracker.signal() (strategies/coinrule/price_tracker.py
    :165-251) for every candle of a 5m panel in one pass
    (engine.price_tracker_replay, bq_price_tracker_replay). Column t of row s
    = the method on the message whose frame is df.iloc[first_t[s]:t + 1],
    after the messages of all earlier candles; candles from_t[s] ..
    lens[s] - 1 are replayed, from `state` (None: no cooldown entry), which is
    updated in place. c / rsi / macd / mfi [S, T] float64 (engine.enrich's
    columns; mfi's column t is Indicators.mfi of the frame ending at t), h / l
    / v only for the tail(5).isnull() test (None: no NaN in them), close_time
    [S, T] int64 ms. trend_score: the method's EMA 9 / 21 score [S, T], or
    None to form it in the pass (1e-9 of pandas). symbol_rs [S] or [S, T]: the
    context snapshot's relative_strength_vs_btc of the symbol, 0.0 where it
    has none. ctx [4, 1] or [4, T] float64 (PT_CTX_ROWS) and ctx_ok [1] / [T]
    (False: latest_market_context is None), both on the device. params:
    engine.PRICE_TRACKER_DEFAULTS' keys.

    Returns {"status": uint8 [S, T] (PT_* codes, PT_REASONS their names; 0 =
    the message goes out and the cooldown entry moves to close_time[t]),
    "detail": uint8 [S, T] (PT_D_* bits of a PT_CONTEXT_REJECTED candle), and
    the `columns` of PT_VALUES, float64 [S, T], NaN where the method did not
    reach them}. regime_routing only sets the message's autotrade flag
    (price_tracker_routing); is_autotrade_suppressed reads the wall clock and
    stays a host step, as do the message text and the dispatch."""
    status, detail, vals = engine.price_tracker_replay(
        c, rsi, macd, mfi, close_time, symbol_rs, ctx, ctx_ok, h=h, l=l, v=v, trend_score=trend_score,
        state=state.tensors() if state is not None else None, first_t=first_t, lens=lens, from_t=from_t,
        columns=columns, **params)
    return {"status": status, "detail": detail, **vals}


def _first_code(checks, none):
    """The code (a float or an expression) beside the first true check."""
    code = none if isinstance(none, F.Ex) else F.const(float(none))
    for cond, value in reversed(checks):
        code = F.where(cond, value if isinstance(value, F.Ex) else float(value), code)
    return code


# PriceTracker.regime_routing's strings (:113-163) as uint8 codes, in the method's order; the three f-string
# families are expanded over their enums (market_regime_range / symbol_regime_range cannot occur)
PT_ROUTE_REASONS = (("market_context_unavailable", "market_transitioning", "market_stress_too_high",
                     "breadth_not_stable_for_mean_reversion", "market_regime_unavailable")
                    + tuple(f"market_regime_{r.lower()}" for r in _lib.MARKET_REGIMES)
                    + ("symbol_regime_unavailable", "symbol_transition_breakdown",
                       "symbol_transition_volatility_expansion", "symbol_relative_strength_vs_btc_insufficient",
                       "symbol_trend_score_outside_range", "symbol_range")
                    + tuple(f"symbol_regime_{r.lower()}" for r in _lib.MICRO_REGIMES))
PT_ROUTE_OK = PT_ROUTE_REASONS.index("symbol_range")


def price_tracker_routing(context_ok, regime_is_transitioning, market_stress_score, advancers_ratio, long_tailwind,
                          short_tailwind, market_regime, features_ok, micro_regime, micro_transition,
                          relative_strength_vs_btc, trend_score, stress_threshold: float = 0.3,
                          min_relative_strength: float = 0.005, max_abs_trend_score: float = 0.005):
    """PriceTracker.regime_routing (strategies/coinrule/price_tracker.py:113-163,
    with _has_stable_breadth :101-111) per (symbol, candle). The context's
    fields [T] (or [S, T]): context_ok / regime_is_transitioning bool,
    market_stress_score / advancers_ratio / long_tailwind / short_tailwind
    float64, market_regime int8 (_lib.MARKET_REGIMES codes, negative: None);
    the symbol's features [S, T]: features_ok bool (False: the context has
    none for the symbol), micro_regime / micro_transition int8
    (_lib.MICRO_REGIMES / MICRO_TRANSITIONS codes, negative: None),
    relative_strength_vs_btc / trend_score float64 (the snapshot's, not the
    frame's EMA score). stress_threshold: min(autotrade_stress_threshold, 0.3)
    (:124). Returns (autotrade_ok bool [S, T], reason uint8 [S, T]): the first
    refusing check in the method's order, PT_ROUTE_REASONS its strings
    (PT_ROUTE_OK = "symbol_range", the accepting route). The verdict only
    sets the emitted message's autotrade flag. One fused element-wise
    program."""
    S, T = trend_score.shape
    R = PT_ROUTE_REASONS.index
    STRESS, AR, LT, ST = (F.inp(x) for x in (market_stress_score, advancers_ratio, long_tailwind, short_tailwind))
    MKT = F.inp(market_regime.to(torch.float64))
    MR, MT = F.inp(micro_regime.to(torch.float64)), F.inp(micro_transition.to(torch.float64))
    RS, TREND = F.inp(relative_strength_vs_btc), F.inp(trend_score)
    stable = (AR >= 0.48) & (AR <= 0.62) & ((LT - ST).abs() <= 0.35)
    rng_mkt, rng_sym = float(_lib.MARKET_REGIMES.index("RANGE")), float(_lib.MICRO_REGIMES.index("RANGE"))
    code = _first_code([
        (~F.inp(context_ok), R("market_context_unavailable")),
        (F.inp(regime_is_transitioning), R("market_transitioning")),
        (STRESS >= float(stress_threshold), R("market_stress_too_high")),
        (~stable, R("breadth_not_stable_for_mean_reversion")),
        (MKT < 0.0, R("market_regime_unavailable")),
        (MKT != rng_mkt, MKT + float(R("market_regime_" + _lib.MARKET_REGIMES[0].lower()))),
        (~F.inp(features_ok), R("symbol_regime_unavailable")),
        (MT == float(_lib.MICRO_TRANSITIONS.index("BREAKDOWN")), R("symbol_transition_breakdown")),
        (MT == float(_lib.MICRO_TRANSITIONS.index("VOLATILITY_EXPANSION")),
         R("symbol_transition_volatility_expansion")),
        (RS <= min_relative_strength, R("symbol_relative_strength_vs_btc_insufficient")),
        (TREND.abs() > max_abs_trend_score, R("symbol_trend_score_outside_range")),
        (MR == rng_sym, PT_ROUTE_OK),
        (MR < 0.0, R("symbol_regime_unavailable")),
    ], MR + float(R("symbol_regime_" + _lib.MICRO_REGIMES[0].lower())))
    reason = F.run({"reason": code}, S, T)["reason"].to(torch.uint8)
    return reason == PT_ROUTE_OK, reason


# allows_long_autotrade's outcomes (market_regime/regime_routing.py:47-75) as uint8 codes: 0 allows, then the first
# refusing check in the function's order (it returns a bare bool: the names are this library's)
LONG_AUTOTRADE_REASONS = ("long_autotrade_allowed", "market_context_unavailable", "market_transitioning",
                          "market_regime_not_stable", "market_regime_blocked", "market_stress_too_high",
                          "market_regime_not_long", "symbol_trend_down_without_recovery", "symbol_volatile",
                          "symbol_regime_not_long")


def long_autotrade_allows(context_ok, regime_is_transitioning, timestamp, regime_stable_since, market_regime,
                          market_stress_score, features_ok, micro_regime, micro_transition,
                          min_age_ms: int = 30 * 60 * 1000, max_market_stress: float = 0.35):
    """allows_long_autotrade with is_regime_stable / regime_age_ms
    (market_regime/regime_routing.py:22-75) per (symbol, candle). The
    context's fields [T] (or [S, T]): context_ok / regime_is_transitioning
    bool, timestamp / regime_stable_since int64 ms (regime_stable_since
    negative: None), market_regime int8 (_lib.MARKET_REGIMES codes, negative:
    None), market_stress_score float64; the symbol's features [S, T]:
    features_ok bool (False: no symbol given or no features for it),
    micro_regime / micro_transition int8 (negative: None). The regime's age
    max(timestamp - regime_stable_since, 0) is formed in int64 before it
    enters the program (exact in float64 below 2^53 ms). Returns (ok bool
    [S, T], reason uint8 [S, T], LONG_AUTOTRADE_REASONS its strings; 0 =
    allowed). One fused element-wise program."""
    S, T = micro_regime.shape
    age = (timestamp - regime_stable_since).clamp_min(0)
    AGE = F.inp(torch.where(regime_stable_since < 0, torch.full_like(age, -1), age).to(torch.float64))
    MKT, STRESS = F.inp(market_regime.to(torch.float64)), F.inp(market_stress_score)
    MR, MT = F.inp(micro_regime.to(torch.float64)), F.inp(micro_transition.to(torch.float64))
    mk, mi, tr = _lib.MARKET_REGIMES.index, _lib.MICRO_REGIMES.index, _lib.MICRO_TRANSITIONS.index
    blocked = ((MKT == float(mk("HIGH_STRESS"))) | (MKT == float(mk("TREND_DOWN")))
               | (MKT == float(mk("TRANSITIONAL"))))
    mkt_long = (MKT == float(mk("TREND_UP"))) | (MKT == float(mk("RANGE")))
    sym_long = ((MR == float(mi("TREND_UP"))) | (MR == float(mi("RANGE"))) | (MR == float(mi("TRANSITIONAL"))))
    FOK = F.inp(features_ok)
    code = _first_code([
        (~F.inp(context_ok), 1), (F.inp(regime_is_transitioning), 2),
        ((AGE < 0.0) | (AGE < float(min_age_ms)), 3),   # no anchor yet, or too young
        (blocked, 4), (STRESS >= max_market_stress, 5),
        (~FOK & ~mkt_long, 6), (~FOK, 0),
        ((MR == float(mi("TREND_DOWN"))) & (MT != float(tr("RECOVERY"))), 7),
        (MR == float(mi("TREND_DOWN")), 0),
        (MR == float(mi("VOLATILE")), 8), (~sym_long, 9),
    ], 0)
    reason = F.run({"reason": code}, S, T)["reason"].to(torch.uint8)
    return reason == 0, reason


# activity_burst_entry's status codes: where ActivityBurstPump.signal() returned (:164-185), in the method's order
(AB_EMIT, AB_NO_FRAME, AB_SHORT_FRAME, AB_ROUTE_REFUSED, AB_NOT_QUALIFIED) = range(5)
AB_REASONS = {AB_EMIT: "emit", AB_NO_FRAME: "no_frame", AB_SHORT_FRAME: "frame_too_short",
              AB_ROUTE_REFUSED: "long_autotrade_refused", AB_NOT_QUALIFIED: "not_qualified"}


def activity_burst_entry(qualified, route_ok, ctx_ok, *, first_t=None, lens=None, min_rows: int = 21):
    """ActivityBurstPump.signal() from its frame gate to the qualified_signal
    test (strategies/activity_burst_pump.py:164-185) per (symbol, candle):
    qualified [S, T] bool (activity_burst_features' qualified_signal; column t
    = the frame ending at t), route_ok [S, T] (or [S, 1] / [T]) bool:
    allows_long_autotrade (long_autotrade_allows), read only where a context
    exists; ctx_ok [T] (or one element) bool: latest_market_context is not
    None. The frame is df.iloc[first_t[s]:t + 1], t < lens[s]; min_rows =
    lookback_window + 1. Returns {"status": uint8 [S, T] (AB_* codes, the
    first return in the method's order; 0 = the message goes out),
    "autotrade": bool [S, T], the emitted message's flag (a context exists)}.
    One fused element-wise program."""
    S, T = qualified.shape
    dev = qualified.device
    tcol = torch.arange(T, dtype=torch.float64, device=dev)
    rows = lambda x, dflt: (torch.full((S, 1), float(dflt), dtype=torch.float64, device=dev) if x is None else
                            torch.as_tensor(x).to(device=dev, dtype=torch.float64).reshape(S, 1))
    FIRST, LEN, TT = F.inp(rows(first_t, 0)), F.inp(rows(lens, T)), F.inp(tcol)
    CTX = F.inp(ctx_ok.reshape(-1) if ctx_ok.numel() == T else ctx_ok.reshape(1, 1))
    code = _first_code([
        ((TT < FIRST) | (TT >= LEN), AB_NO_FRAME), (TT + 1.0 - FIRST < float(min_rows), AB_SHORT_FRAME),
        (CTX & ~F.inp(route_ok), AB_ROUTE_REFUSED), (~F.inp(qualified), AB_NOT_QUALIFIED)], AB_EMIT)
    res = F.run({"status": code, "autotrade": (code == float(AB_EMIT)) & CTX}, S, T)
    return {"status": res["status"].to(torch.uint8), "autotrade": res["autotrade"]}


# ---- the 15m dip buyer: BuyTheDip -----------------------------------------------------------------------------------
# bq_buy_the_dip_replay's status codes: where BuyTheDip.signal() returned, in the method's order (the reference
# returns silently or with a log line: DIP_REASONS' names are this library's)
(DIP_EMIT, DIP_NO_FRAME, DIP_NOT_READY, DIP_BEFORE_START, DIP_NO_REFERENCE, DIP_OUT_OF_BAND, DIP_REGIME_BLOCKED,
 DIP_NOT_RECLAIMED) = range(8)
DIP_REASONS = dict(enumerate(_lib.DIP_REASONS))
DIP_VALUES = _lib.DIP_VALUES


def buy_the_dip_entry(c, close_time, market_regime, micro_regime, *, ema20=None, first_t=None, lens=None, from_t=None,
                      columns=DIP_VALUES, **params):
    """The decisions of BuyTheDip.signal() (strategies/coinrule/buy_the_dip.py
    :127-181) for every candle of a 15m panel in one pass
    (engine.buy_the_dip_replay, bq_buy_the_dip_replay). Column t of row s =
    the method on the message whose frame is df.iloc[first_t[s]:t + 1] with
    current_price = close[t]; candles from_t[s] .. lens[s] - 1 are replayed.
    The method keeps no state: a column does not depend on earlier messages.
    c [S, T] float64, close_time [S, T] int64 ms, strictly ascending within a
    row's frame: the 6 h reference is the newest candle whose close_time is at
    least lookback_ms older than the message's, found by time, so a row with
    a halt gets the candle the method takes and not close[t - 24]. ema20: the
    method's close.ewm(span=20, adjust=False, min_periods=1).mean() [S, T], or
    None to form it in the pass (1e-9 of pandas). market_regime int8 [1] or
    [T] (_lib.MARKET_REGIMES codes; negative: latest_market_context is None,
    or its market_regime is) and micro_regime int8 [S] or [S, T]
    (_lib.MICRO_REGIMES codes; negative: the context has no features for the
    symbol, or their micro_regime is None), both on the device; None: absent
    for every candle. params: engine.BUY_THE_DIP_DEFAULTS' keys.

    Returns {"status": uint8 [S, T] (DIP_* codes, DIP_REASONS their names; 0 =
    the message goes out), and the `columns` of DIP_VALUES, float64 [S, T],
    NaN where the method did not reach them}. _allows_buy_the_dip_autotrade
    and _resolve_autotrade_route only set the message's autotrade flag and
    route (buy_the_dip_routing); is_autotrade_suppressed reads the wall clock
    and stays a host step, as do the message text and the dispatch."""
    status, vals = engine.buy_the_dip_replay(c, close_time, market_regime, micro_regime, ema20=ema20, first_t=first_t,
                                             lens=lens, from_t=from_t, columns=columns, **params)
    return {"status": status, **vals}


# BuyTheDip._resolve_autotrade_route's strings (:106-125) as uint8 codes, in the method's order; the two f-string
# families are expanded over their enums (market_regime_none: the method formats str(None); market_regime_range /
# market_regime_transitional cannot occur)
DIP_ROUTE_REASONS = (("market_context_unavailable", "market_transitioning", "market_stress_too_high")
                     + tuple(f"market_regime_{r.lower()}" for r in _lib.MARKET_REGIMES) + ("market_regime_none",)
                     + ("symbol_regime_unavailable",)
                     + tuple(f"symbol_regime_{r.lower()}" for r in _lib.MICRO_REGIMES))


def buy_the_dip_routing(context_ok, regime_is_transitioning, market_stress_score, market_regime, features_ok,
                        micro_regime, max_market_stress: float = 0.35):
    """BuyTheDip._allows_buy_the_dip_autotrade and _resolve_autotrade_route
    (strategies/coinrule/buy_the_dip.py:87-125) per (symbol, candle). The
    context's fields [T] (or [S, T]): context_ok / regime_is_transitioning
    bool, market_stress_score float64, market_regime int8
    (_lib.MARKET_REGIMES codes, negative: None); the symbol's features [S, T]:
    features_ok bool (False: the context has none for the symbol),
    micro_regime int8 (_lib.MICRO_REGIMES codes, negative: None). Returns
    (autotrade bool [S, T], reason uint8 [S, T]): the emitted message's flag
    and DIP_ROUTE_REASONS' index of its route. The two methods disagree on
    purpose: without features autotrade is True under
    symbol_regime_unavailable, with features whose micro_regime is None it is
    False under the same route. Quiet hours (is_autotrade_suppressed) are the
    host's. One fused element-wise program."""
    S, T = micro_regime.shape
    R = DIP_ROUTE_REASONS.index
    CTX, TRANS, FEAT = F.inp(context_ok), F.inp(regime_is_transitioning), F.inp(features_ok)
    STRESS = F.inp(market_stress_score)
    MKT, MR = F.inp(market_regime.to(torch.float64)), F.inp(micro_regime.to(torch.float64))
    mkt_ok = ((MKT == float(_lib.MARKET_REGIMES.index("RANGE")))
              | (MKT == float(_lib.MARKET_REGIMES.index("TRANSITIONAL"))))
    sym_ok = ((MR == float(_lib.MICRO_REGIMES.index("RANGE")))
              | (MR == float(_lib.MICRO_REGIMES.index("TRANSITIONAL"))))
    stressed = STRESS >= float(max_market_stress)
    code = _first_code([
        (~CTX, R("market_context_unavailable")),
        (TRANS, R("market_transitioning")),
        (stressed, R("market_stress_too_high")),
        (MKT < 0.0, R("market_regime_none")),
        (~mkt_ok, MKT + float(R("market_regime_" + _lib.MARKET_REGIMES[0].lower()))),
        (~FEAT | (MR < 0.0), R("symbol_regime_unavailable")),
    ], MR + float(R("symbol_regime_" + _lib.MICRO_REGIMES[0].lower())))
    auto = CTX & ~TRANS & ~stressed & mkt_ok & (~FEAT | sym_ok)
    res = F.run({"reason": code, "autotrade": auto}, S, T)
    return res["autotrade"], res["reason"].to(torch.uint8)


# ---- the RSI(2) fade at the Bollinger extremes: BBExtremeReversion --------------------------------------------------
# bq_bb_extreme_replay's status codes: where BBExtremeReversion.signal() returned, in the method's order (the names
# restate its log lines and evaluate()'s reasons)
(BBX_EMIT, BBX_NO_FRAME, BBX_NOT_ENOUGH_DATA, BBX_NULLS, BBX_NO_RSI, BBX_INVALID_BAND, BBX_NO_EXTREME) = range(7)
BBX_REASONS = dict(enumerate(_lib.BBX_REASONS))
BBX_VALUES = _lib.BBX_VALUES
BBX_BUY, BBX_SELL = 0.0, 1.0   # the direction column: bq_direction LONG / SHORT


def bb_extreme_entry(c, bb_upper, bb_mid, bb_lower, *, first_t=None, lens=None, from_t=None, columns=BBX_VALUES,
                     **params):
    """The decisions of BBExtremeReversion.signal() (strategies/coinrule/
    bb_extreme_reversion.py:234-285 with evaluate :152-232 and _compute_rsi
    :134-150) for every candle of a 15m panel in one pass
    (engine.bb_extreme_replay, bq_bb_extreme_replay). Column t of row s = the
    method on the message whose frame is df.iloc[first_t[s]:t + 1] with
    current_price = close[t] and bb_high / bb_mid / bb_low = the bands of
    candle t; candles from_t[s] .. lens[s] - 1 are replayed. The method keeps
    no state: a column does not depend on earlier messages. ENABLED is not
    replayed: the panel form answers what the method does when enabled.
    c / bb_upper / bb_mid / bb_lower [S, T] float64. The bands are taken as
    given: the evaluator's round_numbers(.., 6) on bb_spreads is the caller's
    step, applied before the call. The RSI is local to each frame:
    rolling(rsi_window).mean() over the gains and losses of df.tail(lookback)
    is an online sum started at that frame's first row, so its last value
    depends on all `lookback` closes; the pass replays that sum for every
    candle, bit for bit with pandas 2.3.3 (a row-wide rolling mean is a
    different number after a spike). params: engine.BB_EXTREME_DEFAULTS'
    keys.

    Returns {"status": uint8 [S, T] (BBX_* codes, BBX_REASONS their names; 0 =
    the message goes out), and the `columns` of BBX_VALUES, float64 [S, T],
    NaN where the method did not reach evaluate}: rsi_value (50.0 under
    BBX_NO_RSI), band_position, bb_width, distance_from_mid_pct, and direction
    (BBX_BUY / BBX_SELL) on emitted messages alone. supports_autotrade and
    _resolve_directional_autotrade only set the message's autotrade flag and
    route (bb_extreme_routing); the message text, the dispatch and
    process_autotrade_restrictions stay host steps."""
    status, vals = engine.bb_extreme_replay(c, bb_upper, bb_mid, bb_lower, first_t=first_t, lens=lens, from_t=from_t,
                                            columns=columns, **params)
    return {"status": status, **vals}


# supports_autotrade's and _resolve_directional_autotrade's strings (:86-132) as uint8 codes, in the methods' order;
# the f-string families are expanded over their enums (market_regime_none: the method formats str(None);
# market_regime_range cannot occur; only RANGE reaches market_{slug}_unstable_allowed / _stable) and over
# MICRO_REGIME_BLOCKING_TRANSITIONS
BBX_BLOCKING_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKDOWN", "ENTERED_TRANSITIONAL")
BBX_ROUTE_REASONS = (("market_context_unavailable", "market_transitioning", "market_stress_too_high")
                     + tuple(f"market_regime_{r.lower()}" for r in _lib.MARKET_REGIMES) + ("market_regime_none",)
                     + ("market_range_unstable_allowed", "market_range_stable", "symbol_features_unavailable")
                     + tuple(f"symbol_transition_{r.lower()}" for r in BBX_BLOCKING_TRANSITIONS)
                     + ("symbol_micro_regime_unstable", "symbol_regime_not_shortable",
                        "symbol_regime_trend_down_for_long"))


def bb_extreme_routing(context_ok, regime_is_transitioning, timestamp, regime_stable_since, market_stress_score,
                       market_regime, features_ok, micro_regime, micro_transition, micro_regime_strength, direction,
                       stress_threshold: float = 0.35, min_age_ms: int = 30 * 60 * 1000, min_strength: float = 0.5):
    """BBExtremeReversion.supports_autotrade and
    _resolve_directional_autotrade (strategies/coinrule/
    bb_extreme_reversion.py:86-132, with is_regime_stable,
    market_regime/regime_routing.py:22-44) per (symbol, candle). The context's
    fields [T] (or [S, T]): context_ok / regime_is_transitioning bool,
    timestamp / regime_stable_since int64 ms (regime_stable_since negative:
    None), market_stress_score float64, market_regime int8
    (_lib.MARKET_REGIMES codes, negative: None); the symbol's features [S, T]:
    features_ok bool (False: the context has none for the symbol),
    micro_regime / micro_transition int8 (_lib.MICRO_REGIMES /
    MICRO_TRANSITIONS codes, negative: None), micro_regime_strength float64;
    direction float64 [S, T]: bb_extreme_entry's column (BBX_BUY / BBX_SELL;
    NaN, no message: neither directional test applies). The regime's age
    max(timestamp - regime_stable_since, 0) is formed in int64 before it
    enters the program, as long_autotrade_allows forms it. Returns (autotrade
    bool [S, T], route uint8 [S, T]): the emitted message's flag and
    BBX_ROUTE_REASONS' index of its route; an allowed message keeps the market
    route (market_range_unstable_allowed or market_range_stable). As in the
    methods: a NaN micro_regime_strength passes the < min_strength test; a
    None micro regime is not shortable for a sell and allowed for a buy. One
    fused element-wise program."""
    S, T = micro_regime.shape
    R = BBX_ROUTE_REASONS.index
    age = (timestamp - regime_stable_since).clamp_min(0)
    AGE = F.inp(torch.where(regime_stable_since < 0, torch.full_like(age, -1), age).to(torch.float64))
    CTX, TRANS, FEAT = F.inp(context_ok), F.inp(regime_is_transitioning), F.inp(features_ok)
    STRESS, STRENGTH, DIR = F.inp(market_stress_score), F.inp(micro_regime_strength), F.inp(direction)
    MKT = F.inp(market_regime.to(torch.float64))
    MR, MT = F.inp(micro_regime.to(torch.float64)), F.inp(micro_transition.to(torch.float64))
    mi, tr = _lib.MICRO_REGIMES.index, _lib.MICRO_TRANSITIONS.index
    shortable = ((MR == float(mi("RANGE"))) | (MR == float(mi("TRANSITIONAL"))) | (MR == float(mi("TREND_DOWN"))))
    base = F.where((AGE < 0.0) | (AGE < float(min_age_ms)), float(R("market_range_unstable_allowed")),
                   float(R("market_range_stable")))
    refusals = [
        (~CTX, R("market_context_unavailable")),
        (TRANS, R("market_transitioning")),
        (STRESS >= float(stress_threshold), R("market_stress_too_high")),
        (MKT < 0.0, R("market_regime_none")),
        (MKT != float(_lib.MARKET_REGIMES.index("RANGE")),
         MKT + float(R("market_regime_" + _lib.MARKET_REGIMES[0].lower()))),
        (~FEAT, R("symbol_features_unavailable")),
    ] + [(MT == float(tr(name)), R("symbol_transition_" + name.lower())) for name in BBX_BLOCKING_TRANSITIONS] + [
        (STRENGTH < float(min_strength), R("symbol_micro_regime_unstable")),
        ((DIR == BBX_SELL) & ~shortable, R("symbol_regime_not_shortable")),
        ((DIR == BBX_BUY) & (MR == float(mi("TREND_DOWN"))), R("symbol_regime_trend_down_for_long")),
    ]
    refused = refusals[0][0]
    for cond, _ in refusals[1:]:
        refused = refused | cond
    res = F.run({"route": _first_code(refusals, base), "autotrade": ~refused}, S, T)
    return res["autotrade"], res["route"].to(torch.uint8)


# ---- the contrarian long on a relative-strength leader in a weak RANGE market: RelativeStrengthReversalRange ---------
# bq_rs_reversal_replay's status codes: where RelativeStrengthReversalRange.signal() returned, in the method's order
# (3-8: regime_routing's reasons; the others are this library's names)
(RSR_EMIT, RSR_NO_FRAME, RSR_SHORT_FRAME, RSR_NO_CONTEXT, RSR_REGIME_NONE, RSR_NOT_RANGE, RSR_MARKET_NOT_WEAK,
 RSR_NO_FEATURES, RSR_RS_INSUFFICIENT, RSR_DEAD_TAPE) = range(10)
RSR_REASONS = dict(enumerate(_lib.RSR_REASONS))
RSR_VALUES = _lib.RSR_VALUES
RSR_ROUTE = "range_rs_reversal"   # the route of every emitted message; autotrade is always False


def rs_reversal_entry(volume, context_ok, market_regime, average_return, features_ok, rs, *, first_t=None, lens=None,
                      from_t=None, columns=RSR_VALUES, **params):
    """The decisions of RelativeStrengthReversalRange.signal() (strategies/
    relative_strength_reversal_range.py:75-101 with regime_routing :56-73) for
    every candle of a 15m panel in one pass (engine.rs_reversal_replay,
    bq_rs_reversal_replay). Column t of row s = the method on the message
    whose frame is df.iloc[first_t[s]:t + 1]; candles from_t[s] .. lens[s] - 1
    are replayed. The method keeps no state: a column does not depend on
    earlier messages. volume [S, T] float64. The context of candle t's
    message, [1] (one context for every candle) or [T]: context_ok bool /
    uint8 (None: present), market_regime int8 (_lib.MARKET_REGIMES codes,
    negative: None), average_return float64. The symbol's entry in the
    context's snapshot, [S] or [S, T]: features_ok bool / uint8 (None:
    present) and rs, its relative_strength_vs_btc. The volume floor is
    df["volume"].tail(window).quantile(quantile): Series.quantile, numpy's
    linear percentile with its two-sided lerp over the non-NaN rows, +-inf a
    value: not pandas' rolling quantile (a one-sided lerp, +-inf missing),
    which gives another number on many windows. A finite rank
    beside an infinite one gives a NaN floor, and the method emits. The floor
    sits behind the route gate, so the pass sorts only in the 64-candle steps
    where a candle passes it. params: engine.RS_REVERSAL_DEFAULTS' keys.

    Returns {"status": uint8 [S, T] (RSR_* codes, RSR_REASONS their names; 0 =
    the message goes out), and the `columns` of RSR_VALUES, float64 [S, T]}:
    volume_floor, NaN where the method did not reach it (status 1-8). The
    message always carries autotrade=False and the route RSR_ROUTE, so there
    is no routing function; its text, quote_asset_volume and the dispatch stay
    host steps."""
    status, vals = engine.rs_reversal_replay(volume, context_ok, market_regime, average_return, features_ok, rs,
                                             first_t=first_t, lens=lens, from_t=from_t, columns=columns, **params)
    return {"status": status, **vals}


# ---- the 15m grid ladder: LadderDeployer ----------------------------------------------------------------------------
# bq_grid_ladder_replay's status codes: where LadderDeployer.signal() returned, in the method's order (GL_REASONS:
# its "grid_ladder skipped: ..." log lines by their fixed part; "emit" and "no_frame" are this library's names)
(GL_EMIT, GL_NO_FRAME, GL_POLICY, GL_NO_CONTEXT, GL_NOT_RANGE, GL_MICRO_REGIME, GL_SYMBOL_TRANSITION, GL_BELOW_EMAS,
 GL_RS_NOT_POSITIVE, GL_LONG_SCORE_LOW, GL_BB_EXPANDING, GL_PRICE_OUTSIDE, GL_RANGE_WIDTH) = range(13)
GL_REASONS = dict(enumerate(_lib.GL_REASONS))
GL_VALUES = _lib.GL_VALUES
GL_CTX_ROWS = _lib.GL_CTX_ROWS
GL_SYM_KEYS = ("ok", "micro_regime", "micro_transition", "above_ema20", "above_ema50", "rs_vs_btc", "atr_pct")
GL_BLOCKING_TRANSITIONS = ("BREAKDOWN", "VOLATILITY_EXPANSION", "ENTERED_TREND_DOWN")


def grid_ladder_entry(c, bb_upper, bb_mid, bb_lower, ctx, ctx_ok=None, policy_ok=None, *, bands=None, sym=None,
                      first_t=None, lens=None, from_t=None, columns=GL_VALUES, **params):
    """The decisions of LadderDeployer.signal() (strategies/grid/ladder_deployer.py
    :58-187) and the numbers its deployment is built from, for every candle
    of a 15m panel in one pass (engine.grid_ladder_replay,
    bq_grid_ladder_replay). Column t of row s = the method on the message
    whose frame is df_15m.iloc[first_t[s]:t + 1] with current_price =
    close[t]; candles from_t[s] .. lens[s] - 1 are replayed. The method keeps
    no state; ENABLED and the market_type != FUTURES return (:61-67) are the
    caller's. c and the frame's bb_upper / bb_mid / bb_lower (the columns
    _bb_stable iterates over) [S, T] float64. bands: None (the frame's own
    columns are what signal() receives; each is read once) or the (bb_high,
    bb_mid, bb_low) [S, T] float64 the caller formed, e.g. the evaluator's
    round_numbers(.., 6) of bb_spreads: the rounding is the caller's step. ctx
    [2, 1] (one message) or [2, T] float64 (GL_CTX_ROWS: market_regime, an
    index into _lib.MARKET_REGIMES, negative for None, and long_regime_score),
    ctx_ok [1] / [T] (False: latest_market_context is None; None: present) and
    policy_ok [1] / [T] (grid_only_policy.allow_grid_ladder, e.g.
    grid_only_policy's first result; None: allowed), all on the device. sym:
    None (no symbol has features in the snapshot) or {GL_SYM_KEYS: tensor},
    all [S] or all [S, T]: ok (False: resolve_symbol_features gave None),
    micro_regime / micro_transition as uint8 indices into _lib.MICRO_REGIMES /
    _lib.MICRO_TRANSITIONS (_lib.MR_NONE: None), above_ema20 / above_ema50,
    rs_vs_btc, atr_pct. params: engine.GRID_LADDER_DEFAULTS' keys.

    Returns {"status": uint8 [S, T] (GL_* codes, GL_REASONS their names; 0 =
    the deployment goes out), and the `columns` of GL_VALUES, float64 [S, T],
    NaN where the method did not compute them}: bb_change_pct where it reached
    _bb_stable and the walk got to its last line, range_width_pct on
    GL_RANGE_WIDTH and GL_EMIT, breakout_buffer_pct (indicators'
    atr_buffer_pct), breakout_low and breakout_high on GL_EMIT; range_low /
    range_high are the bands passed. autotrade_settings, model_dump,
    datetime.now, GridDeploymentRequest and the dispatch order stay host
    steps."""
    if (not isinstance(ctx, torch.Tensor) or ctx.dtype != torch.float64 or ctx.dim() != 2
            or ctx.shape[0] != len(GL_CTX_ROWS)):
        raise ValueError(f"ctx: expected a float64 tensor of shape {(len(GL_CTX_ROWS), 1)} or "
                         f"{(len(GL_CTX_ROWS), 'T')} (rows {GL_CTX_ROWS})")
    status, vals = engine.grid_ladder_replay(
        c, bb_upper, bb_mid, bb_lower, ctx[0].to(torch.int8), ctx[1], ctx_ok, policy_ok, bands=bands,
        sym=_pick(sym, GL_SYM_KEYS, "sym"), first_t=first_t, lens=lens, from_t=from_t, columns=columns, **params)
    return {"status": status, **vals}


# GridOnlyPolicy.resolve's reasons (market_regime/grid_only_policy.py:121-158) as uint8 codes, in the method's order;
# the f-string family is expanded over the regimes outside GRID_ONLY_REGIMES. An active policy's reason carries the
# breadth source the host chose ("breadth_momentum_<direction>_<source>"): the code names its fixed part
GRID_ONLY_REGIMES = ("RANGE", "TRANSITIONAL")
GRID_POLICY_REASONS = (("market_context_unavailable", "market_regime_unavailable")
                       + tuple(f"market_regime_{r.lower()}" for r in _lib.MARKET_REGIMES if r not in GRID_ONLY_REGIMES)
                       + ("breadth_momentum_unavailable", "breadth_momentum_toward_trend",
                          "breadth_momentum_toward_range", "breadth_momentum_flat"))


def grid_only_policy(context_ok, market_regime, previous, latest):
    """GridOnlyPolicy.resolve (market_regime/grid_only_policy.py:121-158) after
    _breadth_pair, per candle time: context_ok bool [T] (False: the context is
    None), market_regime int8 [T] (_lib.MARKET_REGIMES codes, negative: None),
    previous / latest float64 [T]: the pair _breadth_pair returned (either
    NaN: it returned None). Choosing the breadth source, dropping its
    non-finite values and ordering it by timestamp (:67-119) read a
    server-side series and stay on the host. Returns (allow bool,
    reason uint8 (GRID_POLICY_REASONS' index), momentum_points float64 —
    (latest - previous) * 100 where the policy is active, NaN elsewhere), each
    of market_regime's shape. allow is grid_ladder_entry's policy_ok. One
    fused element-wise program."""
    shape = tuple(market_regime.shape)
    T = int(market_regime.numel())
    R = GRID_POLICY_REASONS.index
    mk = _lib.MARKET_REGIMES.index
    CTX = F.inp(context_ok.to(torch.bool).reshape(-1))
    MKT = F.inp(market_regime.to(torch.float64).reshape(-1))
    PREV, LAT = F.inp(previous.reshape(-1)), F.inp(latest.reshape(-1))
    grid_regime = (MKT == float(mk(GRID_ONLY_REGIMES[0]))) | (MKT == float(mk(GRID_ONLY_REGIMES[1])))
    no_pair = F.isnan(PREV) | F.isnan(LAT)
    la, pa = LAT.abs(), PREV.abs()
    outside = [r for r in _lib.MARKET_REGIMES if r not in GRID_ONLY_REGIMES]
    family = F.const(float(R("market_regime_" + outside[0].lower())))   # market_regime_<name>, by the regime's code
    for r in outside[1:]:
        family = F.where(MKT == float(mk(r)), float(R("market_regime_" + r.lower())), family)
    code = _first_code([
        (~CTX, R("market_context_unavailable")),
        (MKT < 0.0, R("market_regime_unavailable")),
        (~grid_regime, family),
        (no_pair, R("breadth_momentum_unavailable")),
        (la > pa, R("breadth_momentum_toward_trend")),
        (la < pa, R("breadth_momentum_toward_range")),
    ], R("breadth_momentum_flat"))
    allow = CTX & grid_regime & ~no_pair & ((la > pa) | (la < pa))
    res = F.run({"reason": code, "allow": allow, "momentum_points": F.where(allow, (LAT - PREV) * 100.0, NAN)}, 1, T)
    return (res["allow"].reshape(shape), res["reason"].to(torch.uint8).reshape(shape),
            res["momentum_points"].reshape(shape))
