"""Generate the freshness fixture from the REAL reference (carkod/binquant).

    python tests/golden/make_golden_fresh.py     # writes fresh_panel.npz, fresh_context.json

Runs where the reference is mounted only; the shim directory and the
child-process scheme are make_golden.py's (imported, not copied). Only
numbers and names are written.

The feed drives MarketStateStore(max_bars_per_symbol=30) and
LiveMarketContextAccumulator over 64 symbols x 120 timestamps of seeded
walks: at each timestamp store.update for the symbols that have a candle
there (symbol order), then refresh_context_for_timestamp(ts)
(market_regime/market_state_store.py:19-31, :49-54;
live_market_context_accumulator.py:72-84, :95-242). The panel holds

  rows 1-8    late listings, first candles at t = 5 .. 90
  rows 9-12   one halt of 10-40 candles each, then they resume
  rows 13-18  scattered single missing candles
  row 19      delists at t = 60
  row 20      never present
  row 21      first candle at the last timestamp (fresh, no features)
  row 0       BTC, absent at t = 70, 71, 72
  rows 40-63  24 symbols absent together over t = 100 .. 107 (18 of them
              from t = 95: 43 fresh of 62 tracked, under the 0.7 coverage gate
              with more than 40 fresh)

fresh_panel.npz     high / low / close [64, 120] (NaN = no candle), timestamps
fresh_context.json  every context (null where the reference returns None),
                    per-symbol symbol_features at three timestamps only
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg   # noqa: E402  (shim writer + reference location)

S, T, MAX_BARS, SEED = 64, 120, 30, 20261019
FEATURE_TS = (50, 71, 119)   # halts under way; BTC stale; the last-timestamp listing


def build_panel():
    import numpy as np

    rng = np.random.default_rng(SEED)
    ret = rng.normal(0.0002, 0.006, (S, T))
    scale = 10 ** rng.uniform(-2, 3, S)
    scale[0] = 60_000.0
    c = scale[:, None] * np.exp(np.cumsum(ret, axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    h = np.maximum(o, c) * (1 + rng.uniform(0, 0.003, (S, T)))
    l = np.minimum(o, c) * (1 - rng.uniform(0, 0.003, (S, T)))
    present = np.ones((S, T), dtype=bool)
    for i, t0 in enumerate((5, 17, 29, 41, 53, 65, 77, 90)):       # late listings
        present[1 + i, :t0] = False
    for i, (a, n) in enumerate(((20, 10), (35, 25), (40, 40), (70, 15))):   # halts
        present[9 + i, a:a + n] = False
    for s in range(13, 19):                                          # single missing candles
        present[s, rng.choice(np.arange(3, 93), 5, replace=False)] = False
    present[19, 60:] = False                                         # delisting
    present[20, :] = False                                           # never present
    present[21, :T - 1] = False                                      # listed at the last timestamp
    present[0, 70:73] = False                                        # BTC gap
    present[40:64, 100:108] = False                                  # 24 absent together
    present[46:64, 95:100] = False
    return o, h, l, c, present


def child(out_dir: Path) -> None:
    import numpy as np

    from market_regime.live_market_context_accumulator import LiveMarketContextAccumulator
    from market_regime.market_state_store import MarketStateStore

    o, h, l, c, present = build_panel()
    syms = ["BTCUSDT"] + [f"F{i:02d}USDT" for i in range(1, S)]
    ts = [1_760_200_000_000 + 900_000 * t for t in range(T)]
    store = MarketStateStore(max_bars_per_symbol=MAX_BARS)
    acc = LiveMarketContextAccumulator(store, btc_symbol="BTCUSDT")
    contexts, feats = [], {}
    near_tie = 0
    for t in range(T):
        for s in range(S):
            if present[s, t]:
                store.update(syms[s], dict(timestamp=ts[t], open=float(o[s, t]), high=float(h[s, t]),
                                           low=float(l[s, t]), close=float(c[s, t]), volume=1.0))
        ctx = acc.refresh_context_for_timestamp(ts[t])
        if ctx is None:
            contexts.append(None)
            continue
        d = ctx.model_dump()
        sf = d.pop("symbol_features")
        d["metadata"] = {k: v for k, v in d["metadata"].items() if k != "fresh_symbols"}
        for f in sf.values():   # exact count comparisons must not sit on a tie
            cl = f["close"]
            if min(abs(cl - f["ema20"]), abs(cl - f["ema50"])) <= 1e-12 * abs(cl) or 0 < abs(f["return_pct"]) < 1e-15:
                near_tie += 1
        if t in FEATURE_TS:
            feats[str(t)] = {k: sf[k] for k in sorted(sf)}
        contexts.append(d)

    # the fixture exercises what it is for (asserted on the reference's own output)
    # symbols fresh at t with at least 2 candles so far: the ones with features
    fresh_n = (present & (np.cumsum(present, axis=1) >= 2)).sum(axis=0)
    built = [d for d in contexts if d is not None]
    assert len(built) >= 20, len(built)
    gated = [t for t in range(T) if contexts[t] is None and fresh_n[t] >= 40]   # only the coverage gate is left
    assert len(gated) >= 5, gated
    stale = [t for t in range(T) if contexts[t] is not None and not present[0, t] and contexts[t]["btc_present"]]
    assert len(stale) >= 1, stale
    assert len({d["total_tracked_symbols"] for d in built}) >= 5
    assert near_tie == 0, f"{near_tie} near-ties: change SEED"
    assert all(str(t) in feats for t in FEATURE_TS), sorted(feats)

    nan = np.where(present, 1.0, np.nan)
    np.savez_compressed(out_dir / "fresh_panel.npz", high=h * nan, low=l * nan, close=c * nan,
                        timestamps=np.array(ts, dtype=np.int64), symbols=np.array(syms))
    with open(out_dir / "fresh_context.json", "w") as f:
        json.dump(dict(max_bars=MAX_BARS, btc="BTCUSDT", symbols=syms, timestamps=ts, contexts=contexts,
                       symbol_features=feats, coverage_gated=gated, stale_btc=stale), f,
                  separators=(",", ":"), default=float)
    print(f"fresh fixture: {len(built)} contexts, {len(gated)} coverage-gated with >= 40 fresh, stale BTC at {stale}")


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(Path(sys.argv[2]))
        return
    if not mg.REFERENCE.exists():
        sys.exit("make_golden_fresh.py runs only where the reference is mounted")
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
