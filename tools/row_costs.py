"""Per-§8-row device timings (diagnostic, GPU): each strategy pipeline and
generic kernel at S symbols x T candles, HIP-event timed on the launch stream.
Usage: python tools/row_costs.py [S] [T] [row ...]   (no row names: every row)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from binquant_amd import engine, signals, strategies
from binquant_amd.synth import device_panel

S = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500
T = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000
p = device_panel(S, T, seed=3)
o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
qv = v * c
btc = c[0].clone()
ts = (1_700_000_000_000 + 900_000 * torch.arange(T, device="cuda", dtype=torch.int64)).expand(S, T).contiguous()
atr = engine.enrich(o, h, l, c, v, columns=("ATR",))["ATR"]
spike_src = torch.rand(S, T, device="cuda") < 0.05   # a source_ok mask of the failed-spike-fade replay


_pump: dict = {}


def sweep_cols():
    """The 13 gate columns of bq_sweep_select, computed once: the pump pipeline's outputs and the close."""
    if not _pump:
        _pump.update(strategies.pump_score_features(o, h, l, c, v, btc))
    return [c if k == "close" else _pump[k] for k in signals.SW_COLUMNS]


def sweep_cross():
    sweep_cols()
    return _pump["score_cross"]


_pt: dict = {}


def price_tracker_cols():
    """PriceTracker's columns, computed once: the enrichment's rsi / macd / mfi, a zero relative strength and one
    context for every candle."""
    if not _pt:
        e = engine.enrich(o, h, l, c, v, columns=("rsi", "macd", "mfi"))
        _pt.update(args=(c, e["rsi"], e["macd"], e["mfi"], ts + 899_999, torch.zeros(S, dtype=torch.float64, device="cuda"),
                         torch.tensor([[0.9], [0.4], [0.3], [0.1]], dtype=torch.float64, device="cuda")))
    return _pt["args"]


_mf: dict = {}


def market_feature_cols():
    """The context build's six feature columns, computed once."""
    if not _mf:
        _mf.update(engine.market_features(h, l, c, max_bars=400))
    return _mf


def timeit(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


rows = {
    "enrich14": lambda: engine.enrich(o, h, l, c, v),
    "market_features": lambda: engine.market_features(h, l, c, max_bars=400),
    "beta_corr": lambda: engine.beta_corr(c, btc, 50),
    "supertrend": lambda: engine.supertrend(h, l, c, atr=atr),
    "rolling_mean20": lambda: engine.rolling(v, 20, "mean"),
    "rolling_median19": lambda: engine.rolling(v, 19, "median", shift=2),
    "rolling_q80": lambda: engine.rolling(v, 80, "quantile", q=0.92, min_periods=20),
    "rolling_std12": lambda: engine.rolling(c, 12, "std"),
    "ewm_alpha": lambda: engine.ewm(c, alpha=1 / 14, min_periods=14),
    "row_quantile": lambda: engine.row_quantile(v, 0.85),
    "activity_burst": lambda: strategies.activity_burst_features(o, h, l, c, v, qv),
    "pump_score": lambda: strategies.pump_score_features(o, h, l, c, v, btc),
    "failed_spike": lambda: strategies.failed_spike_features(o, h, l, c, v, qv),
    # FailedSpikeFade.latest_signal() at every candle: the column stage and bq_spike_frames (T <= 2048)
    "failed_spike_frames": lambda: strategies.failed_spike_frames(o, h, l, c, v, qv),
    # the same under the live store's sliding frame of 301 rows: bq_spike_frames_capped (any T)
    "failed_spike_frames_cap301": lambda: strategies.failed_spike_frames(o, h, l, c, v, qv, frame_cap=301),
    "wilder_rsi": lambda: signals.wilder_rsi(c),
    "adx": lambda: signals.adx(h, l, c),
    "zscore": lambda: signals.zscore(c),
    "top_gainer": lambda: signals.top_gainer_features(o, h, l, c, v, qv),
    # the same inputs in one pass: the 21 values plus entry / status / score / stop_loss_pct
    "top_gainer_entry": lambda: signals.top_gainer_entry(o, h, l, c, v, qv),
    # FailedSpikeFade.signal()'s pending-spike replay, every output column, no market masks
    "spike_fade_replay": lambda: engine.spike_fade_replay(o, h, c, ts, spike_src),
    # LiquidationSweepPump's gate and the cohort winner per candle: the kernel alone over the pump columns, all outputs
    "sweep_select": lambda: engine.sweep_select(sweep_cols(), sweep_cross()),
    # PriceTracker.signal()'s decisions, every output column, the EMA 9 / 21 formed in the pass
    "price_tracker_entry": lambda: signals.price_tracker_entry(*price_tracker_cols(), h=h, l=l, v=v),
    # MeanReversionFade.signal()'s decisions, every output column, the RSI / means / trend score formed in the pass
    # (bb_upper: the close as a stand-in column, one context for every candle, no snapshot)
    "mean_reversion_fade_entry": lambda: signals.mean_reversion_fade_entry(
        o, h, l, c, v, atr, c, ts, torch.tensor([[0.1], [0.2], [0.3], [0.0], [0.0]], dtype=torch.float64,
                                                 device="cuda")),
    # RangeBbRsiMeanReversion.signal()'s decisions, every output column, adx and zscore formed in the pass (rsi: the
    # close as a stand-in column, the bands the close, one RANGE context for every candle, a calm snapshot [S])
    "range_fade_entry": lambda: signals.range_fade_entry(
        o, h, l, c, v, c, c, c, c, torch.tensor([[0.0], [0.1], [2.0]], dtype=torch.float64, device="cuda"),
        sym={"ok": torch.ones(S, dtype=torch.uint8, device="cuda"),
             "micro_regime": torch.full((S,), 2, dtype=torch.uint8, device="cuda"),
             "micro_transition": torch.full((S,), 255, dtype=torch.uint8, device="cuda"),
             "atr_pct": torch.full((S,), 0.01, dtype=torch.float64, device="cuda"),
             "bb_width": torch.full((S,), 0.02, dtype=torch.float64, device="cuda")}),
    # LadderDeployer.signal()'s decisions, every output column (the frame's bands h / c / l as stand-in columns, read
    # once; one passing RANGE context for every candle, a passing snapshot [S])
    "grid_ladder_entry": lambda: signals.grid_ladder_entry(
        c, h, c, l, torch.tensor([[2.0], [0.5]], dtype=torch.float64, device="cuda"),
        sym={"ok": torch.ones(S, dtype=torch.uint8, device="cuda"),
             "micro_regime": torch.full((S,), 2, dtype=torch.uint8, device="cuda"),
             "micro_transition": torch.full((S,), 255, dtype=torch.uint8, device="cuda"),
             "above_ema20": torch.ones(S, dtype=torch.uint8, device="cuda"),
             "above_ema50": torch.ones(S, dtype=torch.uint8, device="cuda"),
             "rs_vs_btc": torch.full((S,), 0.1, dtype=torch.float64, device="cuda"),
             "atr_pct": torch.full((S,), 0.01, dtype=torch.float64, device="cuda")}),
    # every symbol's symbol_features entry, micro regime and transition at every candle (all eleven columns; a dense
    # build's feature columns, every context valid, BTC = row 0)
    "symbol_regime_panel": lambda: engine.symbol_regime_panel(market_feature_cols(), c,
                                                              btc_return=market_feature_cols()["return_pct"][0],
                                                              btc_row=0),
    "resample_1h": lambda: engine.resample(ts, {"open": o, "high": h, "low": l, "close": c, "volume": v},
                                           {"open": "first", "high": "max", "low": "min", "close": "last",
                                            "volume": "sum"}, 3_600_000),
    "align": lambda: engine.align(ts, ts[0], btc),
    "join_returns": lambda: engine.join_returns(ts, c, ts[0], btc, capacity=T),
}
only = sys.argv[3:]
res = {}
for name, fn in rows.items():
    if only and name not in only:
        continue
    try:
        ms = timeit(fn)
        res[name] = {"ms": round(ms, 4), "Gcandles_s": round(S * T / ms / 1e6, 2)}
    except Exception as e:   # noqa: BLE001
        res[name] = {"error": repr(e)[:200]}
    print(name, res[name], flush=True)
os.makedirs("gpurun_out", exist_ok=True)
json.dump({"S": S, "T": T, "rows": res}, open("gpurun_out/row_costs.json", "w"), indent=1)
