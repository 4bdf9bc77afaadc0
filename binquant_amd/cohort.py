"""One message cohort on the device: ContextEvaluator.process_data
(producers/context_evaluator.py:347-512) for every symbol of a 15-minute
cohort at once.

KlinesProvider.aggregate_data (consumers/klines_provider.py:300-380) hands
process_data one symbol's 5m and 15m frames (plus the BTC 15m frame) per
closed kline, and the accumulator's context refresh runs beside it
(klines_provider.py:181-199). In the reference every symbol of a cohort pays
that path on its own — ~56 ms of pandas per symbol (enrichment
5.1 ms x 2 frames, the store features 2.2, the burst / pump / spike
pipelines 9.1 / 9.8 / 24.3). ``process_cohort`` runs the same device work for
all S symbols of the cohort in one call:

* 5m frame: indicators_enrichment (bq_enrich, the 14 columns, :367-369) and
  ActivityBurstPump's features (:380-388), and on request the two 5m
  strategies' decisions (price_tracker, burst_entry below);
* 15m frame: indicators_enrichment (:415), the 1h resample (:403-407, a9),
  dynamic_btc_beta_corr (:424, a11: index-aligned frames) and the BTC
  pct_change(96) (:425-428, a12), and on request BuyTheDip's,
  RelativeStrengthReversalRange's and LadderDeployer's decisions (buy_the_dip,
  rs_reversal, grid_ladder below);
* the context refresh at the cohort's close: the breadth partials of every
  timestamp and the last timestamp's symbol features
  (live_market_context_accumulator.py:95-297, bq_context_partials);
* the 15m strategies' feature pipelines: LiquidationSweepPump,
  FailedSpikeFade, TopGainerEarlyMomentum, GradualGainerRetest's leadership
  (:445-499), and on request the decision bodies built on them (gates,
  retest, top_entry, spike_fade, sweep below).

Nothing reads back to the host, so the whole cohort can be captured once
as a hipGraph (``graphs.CapturedPipeline(process_cohort, ...)``) and
replayed per message; captured, the stages run as four concurrent branches
of the graph (the current stream and three side streams forked from it and
joined before the return; eager calls stay on one stream, see
_COHORT_STREAMS).
Frames share one geometry per call: [S, T5] 5m and [S, T15] 15m panels, the
BTC 15m close index-aligned with the 15m panel (a cohort closes on the same
15-minute grid); the 1h resample's bin count is fixed by T15.
"""

from __future__ import annotations

import torch

from . import engine, signals, strategies

RESAMPLE_AGG = {"open": "first", "high": "max", "low": "min", "close": "last", "volume": "sum"}
HOUR_MS = 3_600_000

# The stages read only the cohort's inputs, so they can run as four
# concurrent branches (the current stream + three side streams forked from it
# and joined back before the return; captured, the joins become graph
# edges). At live shapes most stages are a few hundred waves — a quarter of
# the chip — so overlapping them is what is left to gain on the device:
# 1000 x 400 as a graph 1.03 -> 0.70 ms. Eager calls are bound by the host's
# launches, which the stream switches and record_stream calls lengthen (2.62
# -> 3.66 ms), so by default ("capture") the branches are used only while a
# graph is being captured; True: always, False: never.
_COHORT_STREAMS: bool | str = "capture"
_SIDE: dict[int, list[torch.cuda.Stream]] = {}


def _side_streams(device: torch.device, n: int) -> list[torch.cuda.Stream]:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _SIDE:
        _SIDE[idx] = [torch.cuda.Stream(device=idx) for _ in range(n)]
    return _SIDE[idx][:n]


def process_cohort(o5, h5, l5, c5, v5, o15, h15, l15, c15, v15, ts15, btc_ts15, btc_c15,
                   max_bars: int = 400, exact: bool = True, h1_max_bins: int | None = None,
                   gates: bool = False, retest: signals.RetestState | None = None,
                   retest_risk: torch.Tensor | None = None, top_entry: bool = False,
                   top_risk: torch.Tensor | None = None, spike_fade: signals.SpikeFadeState | None = None,
                   spike_fade_market: tuple | None = None, sweep: bool = False,
                   sweep_route: torch.Tensor | None = None,
                   sweep_symbol_rank: torch.Tensor | None = None,
                   price_tracker: signals.PriceTrackerState | None = None, ct5: torch.Tensor | None = None,
                   price_tracker_ctx: tuple | None = None, price_tracker_rs: torch.Tensor | None = None,
                   burst_entry: bool = False, burst_route: torch.Tensor | None = None,
                   buy_the_dip: bool = False, ct15: torch.Tensor | None = None,
                   dip_regimes: tuple | None = None, rs_reversal: tuple | None = None,
                   grid_ladder: tuple | None = None) -> dict[str, torch.Tensor]:
    """Device outputs of process_data for a cohort: 5m / 15m panels [S, T5] /
    [S, T15] float64, ts15 [S, T15] int64 open times, btc_ts15 / btc_c15 [T15]
    (index-aligned with the 15m panel). exact=True runs the strategy
    pipelines' bit-exact replays (the live path); False their panel mode.
    h1_max_bins: width of the h1.* arrays (default T15 // 4 + 2, every bin
    of a gap-free 15m grid). pandas emits every empty hour of a gap, so a row
    spanning more hours keeps its NEWEST h1_max_bins bins (bq_resample_tail):
    h1.bins is the count written (<= h1_max_bins, bin h1.bins - 1 is the
    row's latest hour) and h1.dropped the oldest bins left out (0 on a
    gap-free grid). gates=True adds, after the 15m frame and on its stream,
    the entry gates of RelativeStrengthImpulseRider (impulse.<key> for
    signals.IR_KEYS and impulse.status, from the 15m panel, e15.ATR and
    ts15 / btc_ts15 / btc_c15; context_evaluator.py:446-454) and of the grid
    ladder (ladder.stable / ladder.change_pct from e15.bb_*); the default
    leaves the returned dict and the launch sequence as they were. retest: the
    cohort's GradualGainerRetest watchlist (signals.RetestState, [S]): the
    body of its signal() (:222-308 of the strategy) runs on the newest 15m
    candle, after the leadership and on its stream, from that state, which is
    updated in place (a captured graph carries it from message to message);
    retest.event / retest.detail / retest.breakout_level [S] are added.
    retest_risk: _risk_allows for that candle, bool [S] (or [S, T15]; None:
    allowed). Without a state the outputs and launches are unchanged.
    top_entry=True adds, after the 15m frame and on its stream,
    TopGainerEarlyMomentum's decisions for every candle (signals.top_gainer_entry
    on the 15m panel, v15 * c15 and e15.ATR, as the top stage reads them):
    topentry.status / topentry.entry (uint8 [S, T15]) and topentry.score /
    topentry.stop_loss_pct (unrounded). top_risk: _risk_profile_allows per
    candle, bool [S, T15] (or [S]; None: allowed). The default leaves the
    returned dict and the launch sequence as they were. spike_fade: the
    cohort's FailedSpikeFade pending spikes (signals.SpikeFadeState, [S]): the
    body of its signal() (:596-695 of the strategy) runs on the newest 15m
    candle, after the spike stage and on its stream — source_spike_allows
    formed from spike.* (the newest column is the frame-ending-here value) —
    from that state, which is updated in place (a captured graph carries it
    from message to message); spikefade.event / spikefade.detail /
    spikefade.bars [S] are added. spike_fade_market: (source_ok, failure_ok)
    of signals.spike_fade_market_allows for that candle, each bool [T15] or
    one element (broadcast; both [S, T15] where the rows see different
    contexts), or None (allowed). Without a state the outputs
    and launches are unchanged. sweep=True adds, after the pump stage and on
    its stream, LiquidationSweepPump's decision for the cohort's message
    (signals.liquidation_sweep_select on pump.* and c15 at the trigger column
    T15 - 2 only: the newest candle is the message): sweep.status (uint8),
    sweep.candidate (bool) and sweep.rank_score [S], and sweep.winner (int64,
    the row the portfolio selector would dispatch, -1: none) /
    sweep.winner_score, one element each. sweep_route: long_entry_routing's
    verdict, bool [S] (or [S, T15]; None: allowed); sweep_symbol_rank: int32
    [S] on the device, the rows' positions in the str order of their symbols
    (None: the row index). Without sweep the outputs and launches are
    unchanged. price_tracker: the cohort's PriceTracker cooldown entries
    (signals.PriceTrackerState, [S]): the decisions of its signal() (:165-251
    of the strategy) run on the newest 5m candle, after the 5m frame's
    enrichment and on its stream, from e5.rsi / e5.macd / e5.mfi, the 5m
    panel and ct5 (the 5m close_time, int64 [S, T5]), from that state, which
    is updated in place (a captured graph carries it from message to message);
    pricetracker.status / detail / local_score / adjusted_score [S] are
    added. price_tracker_ctx: (ctx float64 [4, 1], ctx_ok bool / uint8 [1] or
    None) of signals.price_tracker_entry, device tensors the caller updates in
    place between replays; price_tracker_rs: the snapshot's
    relative_strength_vs_btc per row, float64 [S] (None: 0.0, no symbol is in
    the snapshot). burst_entry=True adds ActivityBurstPump.signal()'s verdict
    for the newest 5m candle (signals.activity_burst_entry on
    burst.qualified_signal): burst.entry_status (uint8) / burst.autotrade
    (bool) [S]. burst_route: allows_long_autotrade per row, bool [S] (or
    [S, T5]; signals.long_autotrade_allows), or None: latest_market_context is
    None (the message goes out without autotrade). buy_the_dip=True adds, after
    the 15m frame and on its stream, BuyTheDip.signal()'s decision for the
    newest 15m candle (signals.buy_the_dip_entry on c15 and ct15, the 15m
    close_time, int64 [S, T15]; the EMA20 is formed in the pass): dip.status
    (uint8) / dip.reference_price / dip.change_6h [S]. dip_regimes:
    (market_regime int8 [1], micro_regime int8 [S]) of
    signals.buy_the_dip_entry, device tensors the caller updates in place
    between replays (either may be None), or None: no context. rs_reversal:
    (context_ok, market_regime, average_return, features_ok, rs) of
    signals.rs_reversal_entry, device tensors the caller updates in place
    between replays (context_ok / features_ok may be None): adds, after the
    15m frame and on its stream, RelativeStrengthReversalRange.signal()'s
    decision for the newest 15m candle on v15: rsr.status (uint8) /
    rsr.volume_floor [S]. grid_ladder: (ctx, ctx_ok, policy_ok, sym) of
    signals.grid_ladder_entry (ctx float64 [2, 1]; ctx_ok / policy_ok bool /
    uint8 [1] or None; sym a {signals.GL_SYM_KEYS: [S] tensor} dictionary or
    None), device tensors the caller updates in place between replays: adds,
    after the 15m frame and on its stream, LadderDeployer.signal()'s decision
    for the newest 15m candle on c15 and e15.bb_* (the bands unrounded):
    gridladder.status (uint8) and gridladder.<name> for signals.GL_VALUES [S].
    Without these keywords the outputs and launches are unchanged (gates=True's
    ladder.* included). Returns a flat dict of tensors (names prefixed by the
    stage)."""
    S, T15 = c15.shape
    B1 = T15 // 4 + 2 if h1_max_bins is None else int(h1_max_bins)
    btc_c = btc_c15.reshape(-1)

    def frame_5m(out):   # :364-388
        for k, v in engine.enrich(o5, h5, l5, c5, v5).items():
            out[f"e5.{k}"] = v
        for k, v in strategies.activity_burst_features(o5, h5, l5, c5, v5, v5 * c5).items():
            out[f"burst.{k}"] = v
        T5, dev = c5.shape[1], c5.device
        if price_tracker is not None:   # signal()'s decisions on the cohort's message: the newest candle only
            if ct5 is None or price_tracker_ctx is None:
                raise ValueError("process_cohort: price_tracker needs ct5 and price_tracker_ctx")
            ctx, ctx_ok = price_tracker_ctx
            rs = price_tracker_rs if price_tracker_rs is not None else torch.zeros(S, dtype=torch.float64, device=dev)
            newest = torch.full((S,), T5 - 1, dtype=torch.int64, device=dev)
            pt = signals.price_tracker_entry(c5, out["e5.rsi"], out["e5.macd"], out["e5.mfi"], ct5, rs, ctx, ctx_ok,
                                             h=h5, l=l5, v=v5, state=price_tracker, from_t=newest,
                                             columns=("local_score", "adjusted_score"))
            for k in ("status", "detail", "local_score", "adjusted_score"):
                out[f"pricetracker.{k}"] = pt[k][:, -1]
        if burst_entry:   # signal()'s frame gate, routing and qualified_signal (:164-185) on the newest candle
            present = burst_route is not None
            route = burst_route if present else torch.ones((S, 1), dtype=torch.bool, device=dev)
            if route.dim() == 1:
                route = route.reshape(S, 1)
            be = signals.activity_burst_entry(out["burst.qualified_signal"], route,
                                              torch.full((1,), present, dtype=torch.bool, device=dev))
            out["burst.entry_status"], out["burst.autotrade"] = be["status"][:, -1], be["autotrade"][:, -1]

    def frame_15m(out):   # :402-432
        for k, v in engine.enrich(o15, h15, l15, c15, v15).items():
            out[f"e15.{k}"] = v
        bins, res, nbins = engine.resample(ts15, {"open": o15, "high": h15, "low": l15, "close": c15,
                                                  "volume": v15}, RESAMPLE_AGG, HOUR_MS, max_bins=B1, tail=True)
        out["h1.open_time"] = bins
        out["h1.bins"] = nbins.clamp(max=B1)
        out["h1.dropped"] = (nbins - B1).clamp(min=0)
        for k, v in res.items():
            out[f"h1.{k}"] = v
        bc = engine.beta_corr(c15, btc_c15, 50)
        out["btc.beta"], out["btc.corr"] = bc["beta"][:, -1], bc["corr"][:, -1]
        # pct_change(96) with pandas' default pad fill (context_evaluator.py:427-430)
        out["btc.change_24h"] = engine.pct_change(btc_c15.reshape(1, -1), 96)[0, -1:] * 100.0
        if gates:   # :446-454 and the grid ladder's frame scan; no host sync (btc_ts15 is the cohort's own grid)
            feats, status = signals.impulse_rider_features(o15, h15, l15, c15, out["e15.ATR"], ts15,
                                                           btc_ts15.reshape(-1), btc_c, check_bench=False)
            for k, v in feats.items():
                out[f"impulse.{k}"] = v
            out["impulse.status"] = status
            for k, v in signals.bb_width_stable(out["e15.bb_upper"], out["e15.bb_mid"], out["e15.bb_lower"]).items():
                out[f"ladder.{k}"] = v
        if top_entry:   # TopGainerEarlyMomentum.signal() (:363-406 of the strategy) at every candle
            risk = top_risk
            if risk is not None and risk.dim() == 1:
                risk = risk.reshape(S, 1).expand(S, T15)
            te = signals.top_gainer_entry(o15, h15, l15, c15, v15, v15 * c15, out["e15.ATR"], risk_ok=risk,
                                          columns=())
            for k in ("status", "entry", "score", "stop_loss_pct"):
                out[f"topentry.{k}"] = te[k]
        if buy_the_dip:   # BuyTheDip.signal() (:127-181 of the strategy) on the cohort's message: the newest candle only
            if ct15 is None:
                raise ValueError("process_cohort: buy_the_dip needs ct15")
            mkt, micro = dip_regimes if dip_regimes is not None else (None, None)
            newest = torch.full((S,), T15 - 1, dtype=torch.int64, device=c15.device)
            dip = signals.buy_the_dip_entry(c15, ct15, mkt, micro, from_t=newest,
                                            columns=("reference_price", "change_6h"))
            for k in ("status", "reference_price", "change_6h"):
                out[f"dip.{k}"] = dip[k][:, -1]
        if rs_reversal is not None:   # RelativeStrengthReversalRange.signal() (:75-101) on the newest candle only
            cok, mkt, avg, fok, rs = rs_reversal
            newest = torch.full((S,), T15 - 1, dtype=torch.int64, device=c15.device)
            rsr = signals.rs_reversal_entry(v15, cok, mkt, avg, fok, rs, from_t=newest)
            out["rsr.status"], out["rsr.volume_floor"] = rsr["status"][:, -1], rsr["volume_floor"][:, -1]
        if grid_ladder is not None:   # LadderDeployer.signal() (:68-151) on the cohort's message: the newest candle only
            ctx, ctx_ok, policy_ok, sym = grid_ladder
            newest = torch.full((S,), T15 - 1, dtype=torch.int64, device=c15.device)
            gl = signals.grid_ladder_entry(c15, out["e15.bb_upper"], out["e15.bb_mid"], out["e15.bb_lower"], ctx,
                                           ctx_ok, policy_ok, sym=sym, from_t=newest)
            for k in ("status",) + signals.GL_VALUES:
                out[f"gridladder.{k}"] = gl[k][:, -1]

    def context(out):   # klines_provider.py:181-199
        part, last = engine.context_partials(h15, l15, c15, max_bars=max_bars, last=True)
        out["context.partial"] = part
        for k, v in last.items():
            out[f"context.{k}"] = v

    def pump(out):   # :445-499
        for k, v in strategies.pump_score_features(o15, h15, l15, c15, v15, btc_c, exact=exact).items():
            out[f"pump.{k}"] = v
        if sweep:   # signal()'s decision on df.iloc[-2] of the cohort's message, and the selector's pick
            if T15 < 2:
                raise ValueError("process_cohort: sweep needs T15 >= 2 (the trigger candle is T15 - 2)")
            route = sweep_route
            if route is not None and route.dim() == 1:
                route = route.reshape(S, 1).expand(S, T15).contiguous()
            u = T15 - 2
            status, rank, winner, wscore = engine.sweep_select(
                [c15 if k == "close" else out[f"pump.{k}"] for k in signals.SW_COLUMNS], out["pump.score_cross"],
                route_ok=route, symbol_rank=sweep_symbol_rank, t_range=(u, u + 1))
            out["sweep.status"], out["sweep.rank_score"] = status[:, u], rank[:, u]
            out["sweep.candidate"] = out["sweep.status"] == 0
            out["sweep.winner"], out["sweep.winner_score"] = winner[u:u + 1], wscore[u:u + 1]

    def spike(out):
        for k, v in strategies.failed_spike_features(o15, h15, l15, c15, v15, v15 * c15, exact=exact).items():
            out[f"spike.{k}"] = v
        if spike_fade is not None:   # signal()'s body on the cohort's message: the newest candle only
            ok, _ = signals.spike_source_allows(*(out[f"spike.{k}"] for k in (
                "label", "price_break_flag", "cumulative_price_break_flag", "accel_spike_flag", "close_open_ratio",
                "upward")))
            src_m, fail_m = (None if m is None else m if m.dim() == 2 else m.reshape(-1).expand(T15)
                             for m in (spike_fade_market or (None, None)))
            newest = torch.full((S,), T15 - 1, dtype=torch.int64, device=c15.device)
            fs = signals.failed_spike_fade(o15, h15, c15, ts15, ok, src_market=src_m, fail_market=fail_m,
                                           state=spike_fade, from_t=newest)
            for k in ("event", "detail", "bars"):
                out[f"spikefade.{k}"] = fs[k][:, -1]

    def top(out):
        feats, status = signals.top_gainer_features(o15, h15, l15, c15, v15, v15 * c15)
        for k, v in feats.items():
            out[f"top.{k}"] = v
        out["top.status"] = status

    def lead(out):
        res = signals.gradual_gainer_leadership(ts15, c15, btc_ts15, btc_c)
        for k, v in res.items():
            out[f"lead.{k}"] = v
        if retest is not None:   # signal()'s body on the cohort's message: the newest candle only
            risk = retest_risk
            if risk is not None and risk.dim() == 1:
                risk = risk.reshape(S, 1).expand(S, T15)
            newest = torch.full((S,), T15 - 1, dtype=torch.int64, device=c15.device)
            rt = signals.gradual_gainer_retest(o15, h15, l15, c15, ts15, btc_ts15, btc_c, risk_ok=risk, state=retest,
                                               from_t=newest, leadership=res)
            out["retest.event"], out["retest.detail"] = rt["event"][:, -1], rt["detail"][:, -1]
            out["retest.breakout_level"] = rt["breakout_level"][:, -1]

    order = (frame_5m, frame_15m, context, pump, spike, top, lead)
    parts = {f: {} for f in order}
    branches = _COHORT_STREAMS is True or (_COHORT_STREAMS == "capture"
                                            and torch.cuda.is_current_stream_capturing())
    if not branches:
        for f in order:
            f(parts[f])
    else:
        main = torch.cuda.current_stream(c15.device)
        sides = _side_streams(c15.device, 3)
        groups = ((main, (frame_5m, lead)), (sides[0], (frame_15m, context)), (sides[1], (pump, top)),
                  (sides[2], (spike,)))
        for st in sides:
            st.wait_stream(main)
        for st, fs in groups:
            with torch.cuda.stream(st):
                for f in fs:
                    f(parts[f])
        for st in sides:
            main.wait_stream(st)
        for st, fs in groups[1:]:   # outputs made on a side stream are used on the caller's
            for f in fs:
                for v in parts[f].values():
                    v.record_stream(main)
    out: dict[str, torch.Tensor] = {}
    for f in order:
        out.update(parts[f])
    return out
