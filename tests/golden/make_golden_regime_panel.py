"""Generate the per-symbol regime fixture from the REAL reference (carkod/binquant).

    python tests/golden/make_golden_regime_panel.py     # writes regime_panel.npz

Runs where the reference is mounted only; the shim directory and the
child-process scheme are make_golden.py's, as make_golden_fresh.py uses them
(imported, not copied). Only numbers and names are written.

The feed is make_golden_fresh.py's: MarketStateStore(max_bars_per_symbol=30)
and LiveMarketContextAccumulator over regime_panel_gen.py's 64 x 120 panel —
at each timestamp store.update for the symbols that have a candle there
(symbol order), then refresh_context_for_timestamp(ts), which annotates the
new context against the latest one stored before it
(live_market_context_accumulator.py:72-93, regime_transitions.py:25-43).

regime_panel.npz
  exists [T] bool          a context was built at t
  latest [T] int32         the column of KlinesProvider.latest_market_context
                           after t's refresh (consumers/klines_provider.py
                           :193-199), -1 while there is none
  has [S, T] bool          the symbol has an entry in context t's symbol_features
  micro_regime / micro_transition [S, T] int8   indices into the names
                           lists, -1 for None / no entry
  micro_regime_strength, micro_transition_strength, rs_vs_btc [S, T] float64
  above_ema20, above_ema50 [S, T] bool
  return_pct, trend_score, atr_pct, bb_width [S, T] float64   the reference's
                           own feature values (NaN without an entry)
  regimes, transitions     the names the codes index
  timestamps, symbols
"""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg   # noqa: E402  (shim writer + reference location)
import regime_panel_gen as gen   # noqa: E402

REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
               "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")


def child(out_dir: Path) -> None:
    import numpy as np

    from market_regime.live_market_context_accumulator import LiveMarketContextAccumulator
    from market_regime.market_state_store import MarketStateStore

    S, T = gen.S, gen.T
    o, h, l, c, present = gen.build_panel()
    syms = ["BTCUSDT"] + [f"F{i:02d}USDT" for i in range(1, S)]
    ts = [int(x) for x in gen.timestamps()]
    store = MarketStateStore(max_bars_per_symbol=gen.MAX_BARS)
    acc = LiveMarketContextAccumulator(store, btc_symbol="BTCUSDT")
    exists = np.zeros(T, dtype=bool)
    latest = np.full(T, -1, dtype=np.int32)
    has = np.zeros((S, T), dtype=bool)
    code = {k: np.full((S, T), -1, dtype=np.int8) for k in ("micro_regime", "micro_transition")}
    flag = {k: np.zeros((S, T), dtype=bool) for k in ("above_ema20", "above_ema50")}
    val = {k: np.full((S, T), np.nan) for k in ("micro_regime_strength", "micro_transition_strength", "rs_vs_btc",
                                                "return_pct", "trend_score", "atr_pct", "bb_width", "close", "ema20",
                                                "ema50")}
    seen = None          # the provider's latest_market_context, as a column
    absent_from_prev = 0
    for t in range(T):
        for s in range(S):
            if present[s, t]:
                store.update(syms[s], dict(timestamp=ts[t], open=float(o[s, t]), high=float(h[s, t]),
                                           low=float(l[s, t]), close=float(c[s, t]), volume=1.0))
        prev_ctx = acc._get_previous_context(ts[t])
        ctx = acc.refresh_context_for_timestamp(ts[t])
        # KlinesProvider._refresh_latest_market_context (:193-199)
        if ctx is not None:
            seen = t
        elif seen is None:
            lc = acc.get_latest_context()
            seen = ts.index(int(lc.timestamp)) if lc is not None else None
        latest[t] = -1 if seen is None else seen
        if ctx is None:
            continue
        exists[t] = True
        for name, f in ctx.symbol_features.items():
            s = syms.index(name)
            has[s, t] = True
            code["micro_regime"][s, t] = REGIMES.index(f.micro_regime)
            tr = f.micro_regime_transition
            code["micro_transition"][s, t] = -1 if tr is None else TRANSITIONS.index(tr)
            flag["above_ema20"][s, t] = bool(f.above_ema20)
            flag["above_ema50"][s, t] = bool(f.above_ema50)
            val["micro_regime_strength"][s, t] = f.micro_regime_strength
            val["micro_transition_strength"][s, t] = f.micro_regime_transition_strength
            val["rs_vs_btc"][s, t] = f.relative_strength_vs_btc
            for k in ("return_pct", "trend_score", "atr_pct", "bb_width", "close", "ema20", "ema50"):
                val[k][s, t] = getattr(f, k)
            if prev_ctx is not None and name not in prev_ctx.symbol_features:
                absent_from_prev += 1

    # the fixture exercises what it is for (asserted on the reference's own output)
    cells = has.sum()
    counts = {r: int((code["micro_regime"][has] == i).sum()) for i, r in enumerate(REGIMES)}
    events = {e: int((code["micro_transition"][has] == i).sum()) for i, e in enumerate(TRANSITIONS)}
    assert all(counts.values()), counts
    assert all(events.values()), events
    assert absent_from_prev >= 20, absent_from_prev
    idx = np.flatnonzero(exists)
    after_gap = [int(b) for a, b in zip(idx[:-1], idx[1:]) if b != a + 1]
    assert after_gap, "no valid context follows a gated stretch"
    assert (latest[exists] == idx).all() and (np.diff(latest) >= 0).all()
    near = gen.near_cut(val["trend_score"], flag["above_ema20"], flag["above_ema50"], val["rs_vs_btc"],
                        val["bb_width"], val["atr_pct"], val["return_pct"], val["close"], val["ema20"], val["ema50"])
    assert int(near[has].sum()) == 0, f"{int(near[has].sum())} cells within {gen.CUT_EPS} of a cut: change SEED"

    np.savez_compressed(
        out_dir / "regime_panel.npz", exists=exists, latest=latest, has=has, **code, **flag,
        **{k: v for k, v in val.items() if k not in ("close", "ema20", "ema50")},
        regimes=np.array(REGIMES), transitions=np.array(TRANSITIONS), timestamps=np.array(ts, dtype=np.int64),
        symbols=np.array(syms), max_bars=np.int64(gen.MAX_BARS))
    print(f"regime panel fixture: {int(exists.sum())} contexts, {int(cells)} cells, regimes {counts}, "
          f"transitions {events}, {absent_from_prev} cells absent from the predecessor context, "
          f"contexts after a gated stretch at {after_gap}")


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(Path(sys.argv[2]))
        return
    if not mg.REFERENCE.exists():
        sys.exit("make_golden_regime_panel.py runs only where the reference is mounted")
    with tempfile.TemporaryDirectory(prefix="bq_shim_") as tmp:
        shim = Path(tmp)
        mg.write_shim(shim)
        env = dict(os.environ)
        env["PYTHONPATH"] = f"{shim}:{mg.REFERENCE}"
        env["PYTHONDONTWRITEBYTECODE"] = "1"
        env["ENV"] = "ci"
        env["PYTHONHASHSEED"] = "0"   # the accumulator iterates symbol sets: fixed order, stable last bits
        subprocess.run([sys.executable, __file__, "--child", str(HERE)], check=True, env=env, cwd=tmp)


if __name__ == "__main__":
    main()
