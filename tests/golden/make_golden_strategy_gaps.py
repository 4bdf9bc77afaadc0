"""Generate strategy_gaps.npz from the REAL reference (carkod/binquant).

    python tests/golden/make_golden_strategy_gaps.py     # writes strategy_gaps.npz, strategy_gaps_fsf.npz

(one fixture in two files, 1.8 MB together: strategy_gaps_fsf.npz holds the
short rows' fsf__* columns, strategy_gaps.npz everything else; tests/strategy_gaps.py
loads them as one mapping)

Runs where the reference is mounted only; the shim directory and the
child-process scheme are make_golden.py's (imported, not copied). Only
numeric inputs and outputs are written.

Rows with missing candles (tests/golden/strategy_gaps_panel_gen.py: 17 short
rows of 200 candles, 4 long rows of 1100 around the 1024-candle tile edge, a
benchmark with missing candles) through

  abp__*  ActivityBurstPump.compute_indicators    strategies/activity_burst_pump.py:51-158
  lsp__*  LiquidationSweepPump.compute_pump_score strategies/liquidation_sweep_pump.py:195-269
  fsf__*  FailedSpikeFade.detect                  strategies/failed_spike_fade.py:258-544
          fsf_calibrated: (volume_cluster_min_ratio, price_break_base_threshold) after detect()
  a20__*  MeanReversionFade._rsi / _trend_score (mean_reversion_fade.py:88-155),
          RangeBbRsiMeanReversion._compute_adx / _compute_zscore
          (range_bb_rsi_mean_reversion.py:101-138) on prefix frames df.iloc[:t + 1]
          at a20_positions (the last two candles and every candle within 25 of
          a gap edge; -1 pads the ragged rows, NaN pads the values)

Keys: short__<column> [17, 200] (every candle), long__<column> [4, 140]
(candles 960..1099), short__/long__<input field>, *_bench_keep / *_bench_close,
flags as uint8, digest, pandas_version, cases, and the generator's own
findings: fire__<column> [rows] = the column's count after the row's last
gap, score_cross_scattered_sum, std_drift_cells.

Odd rows carry no quote_asset_volume into compute_indicators (their
baseline_quote_volume columns are absent from the reference's frame and stored
as the volume baselines, as the device returns them). FailedSpikeFade needs the
column, so every row has it there.

Checks (fail loudly):
  * qualified_signal, score_cross and label fire after the last gap of every
    gap row, except where no candle after it can: nan_tail (the gap ends the
    row; all three), close_w_pump (score_cross needs a finite threshold at
    t - 1 and t, and only T-1 has one), long_run_1020 and long_run_halo
    (score_cross: the 20-bar volume mean and the 48-bar threshold need 68
    candles after 1030, the row has 69) and scattered_nan_high (score_cross:
    the 48-bar threshold never sees 48 finite scores; its sum, 0, is recorded).
    suppressed_label fires on at least three rows.
  * pandas' own drift stays under half the cap of tests/spike_std.py
    (max_frac = 0.01): per std column, the recorded cells where pandas differs
    from oracle.indicators_ref.exact_std of the window by more than 1e-9
    relative are fewer than 0.5 % of the column's cells.
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

FLAG_DTYPES = ("bool", "int64", "int32", "int8", "uint8", "object")   # object: label after apply_cooldown's .at writes
FIRE = ("qualified_signal", "score_cross", "label")
NO_FIRE = {"nan_tail": FIRE, "close_w_pump": ("score_cross",), "scattered_nan_high": ("score_cross",),
           "long_run_1020": ("score_cross",), "long_run_halo": ("score_cross",)}


def child(out_dir: Path) -> None:
    import warnings
    from types import SimpleNamespace

    import numpy as np
    import pandas as pd

    import strategy_gaps_panel_gen as gen

    sys.path.insert(0, str(HERE.parent.parent))
    from oracle.indicators_ref import exact_std

    from strategies.activity_burst_pump import ActivityBurstPump
    from strategies.failed_spike_fade import FailedSpikeFade
    from strategies.liquidation_sweep_pump import LiquidationSweepPump
    from strategies.mean_reversion_fade import MeanReversionFade
    from strategies.range_bb_rsi_mean_reversion import RangeBbRsiMeanReversion

    ctx_ns = SimpleNamespace(config=SimpleNamespace(env="test"), symbol="TESTUSDT", kucoin_symbol="TEST-USDT",
                             exchange=None, binbot_api=None, telegram_consumer=None, market_type=None,
                             at_consumer=None, _breadth_cross_tolerance=0.05, _autotrade_stress_threshold=0.35,
                             current_symbol_data=None, price_precision=8, qty_precision=8)
    abp = ActivityBurstPump(ctx_ns)
    lsp = object.__new__(LiquidationSweepPump)
    panels = {"short": (gen.short_panel(), gen.SHORT_CASES, gen.T_SHORT, 0),
              "long": (gen.long_panel(), gen.LONG_CASES, gen.T_LONG, gen.LONG_FROM)}
    out: dict[str, np.ndarray] = {
        "digest": np.array(gen.digest(panels["short"][0], panels["long"][0])),
        "pandas_version": np.array(pd.__version__),
        "cases": np.array(gen.SHORT_CASES + gen.LONG_CASES),
    }
    fire = {k: [] for k in FIRE + ("suppressed_label",)}
    drift = {}
    row0 = 0
    for tag, (P, cases, T, lo) in panels.items():
        S = len(cases)
        keep, bench = gen.bench_series(T)
        open_time = 1_700_000_000_000 + 900_000 * np.arange(T, dtype=np.int64)
        dfb = pd.DataFrame({"open_time": open_time[keep], "close": bench[keep]})
        out[f"{tag}__bench_keep"] = keep
        out[f"{tag}__bench_close"] = bench
        for f in gen.FIELDS:
            out[f"{tag}__{f}"] = P[f]
        rec: dict[str, list] = {}
        flags: set[str] = set()
        calib = np.zeros((S, 2))
        pos = [gen.a20_positions(c, T, lo) for c in cases]
        K = max(len(p) for p in pos)
        a20_pos = np.full((S, K), -1, dtype=np.int64)
        a20 = {k: np.full((S, K), np.nan) for k in ("rsi", "trend_score", "adx", "zscore")}

        def put(name, s, series):
            if str(series.dtype) in FLAG_DTYPES:
                flags.add(name)
            rec.setdefault(name, [None] * S)[s] = np.asarray(series, dtype=float)

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            warnings.simplefilter("ignore", FutureWarning)   # pct_change's default fill_method='pad'
            for s, case in enumerate(cases):
                o, h, l, c, v, qv = (P[f][s] for f in gen.FIELDS)
                df = pd.DataFrame({"open": o, "high": h, "low": l, "close": c, "volume": v})
                quote = gen.has_quote(row0 + s)
                if quote:
                    df["quote_asset_volume"] = qv
                res = abp.compute_indicators(df.copy())
                assert len(res) == T
                for col, ser in res.items():
                    if col not in df.columns:
                        put(f"abp__{col}", s, ser)
                if not quote:
                    put("abp__baseline_quote_volume", s, res["baseline_volume"])
                    put("abp__baseline_quote_volume_safe", s, res["baseline_volume_safe"])
                dfl = pd.DataFrame({"open_time": open_time, "open": o, "high": h, "low": l, "close": c, "volume": v})
                res = lsp.compute_pump_score(dfl, dfb)
                assert len(res) == T
                for col, ser in res.items():
                    if col not in dfl.columns:
                        put(f"lsp__{col}", s, ser)
                dff = pd.DataFrame({"open": o, "high": h, "low": l, "close": c, "volume": v,
                                    "quote_asset_volume": qv})
                ns = SimpleNamespace(symbol="TESTUSDT", market_type=None, df_15m=dff.copy(), telegram_consumer=None,
                                     at_consumer=None, current_symbol_data=None, price_precision=8,
                                     market_breadth_data=None, strategy_cooldowns={}, strategy_states={})
                fsf = FailedSpikeFade(ns)
                res = fsf.detect()
                assert len(res) == T
                for col, ser in res.items():
                    if col not in dff.columns:
                        put(f"fsf__{col}", s, ser)
                calib[s] = [fsf.volume_cluster_min_ratio, fsf.price_break_base_threshold]
                # pandas' drift in the five std columns at the recorded cells
                bsp = rec["fsf__body_size_pct"][s]
                for name, x, w, got in (
                        ("price_std", c, 12, rec["fsf__price_std"][s]),
                        ("volume_std", v, 12, pd.Series(v).rolling(12).std().to_numpy()),
                        ("rolling_price_std_8", c, 8, rec["fsf__rolling_price_std_8"][s]),
                        ("rolling_price_std_20", c, 20, rec["fsf__rolling_price_std_20"][s]),
                        ("body_size_pct_std_10", bsp, 10, rec["fsf__body_size_pct_std_10"][s])):
                    n_bad, n = drift.get(name, (0, 0))
                    for t in range(lo, T):
                        n += 1
                        if np.isnan(got[t]):
                            continue
                        ex = exact_std(x[t - w + 1 : t + 1])
                        n_bad += abs(got[t] - ex) > 1e-9 * abs(ex)
                    drift[name] = (n_bad, n)
                # a20 helpers on prefix frames
                a20_pos[s, : len(pos[s])] = pos[s]
                rsi = MeanReversionFade._rsi(pd.Series(c)).to_numpy(dtype=float)
                dft = pd.DataFrame({"open": o, "high": h, "low": l, "close": c, "volume": v})
                for j, t in enumerate(pos[s]):
                    a20["rsi"][s, j] = rsi[t]
                    a20["trend_score"][s, j] = MeanReversionFade._trend_score(dft["close"].iloc[: t + 1])
                    a20["adx"][s, j] = RangeBbRsiMeanReversion._compute_adx(dft.iloc[: t + 1], 14)
                    a20["zscore"][s, j] = RangeBbRsiMeanReversion._compute_zscore(dft.iloc[: t + 1], 20)
                lg = gen.last_gap(case)
                for k, col in (("qualified_signal", "abp__qualified_signal"), ("score_cross", "lsp__score_cross"),
                               ("label", "fsf__label"), ("suppressed_label", "fsf__suppressed_label")):
                    fire[k].append(int(rec[col][s][lg + 1 :].sum()))
                print(f"{case}: last gap {lg}, after it "
                      + ", ".join(f"{k} {fire[k][-1]}" for k in fire) + f", {len(pos[s])} a20 positions")
        for k, rows in rec.items():
            a = np.stack(rows)[:, lo:]
            if k in flags:
                assert np.isin(a, (0.0, 1.0)).all(), k
                a = a.astype(np.uint8)
            out[f"{tag}__{k}"] = a
        out[f"{tag}__fsf_calibrated"] = calib
        out[f"{tag}__a20_positions"] = a20_pos
        for k, a in a20.items():
            out[f"{tag}__a20__{k}"] = a
        row0 += S
    cases = gen.SHORT_CASES + gen.LONG_CASES
    for k in fire:
        out[f"fire__{k}"] = np.array(fire[k], dtype=np.int64)
    for i, case in enumerate(cases):
        if case in gen.CLEAN:
            continue
        for k in FIRE:
            if k in NO_FIRE.get(case, ()):
                continue
            assert fire[k][i] > 0, f"{case}: {k} never fires after the last gap"
    assert sum(n > 0 for n in fire["suppressed_label"]) >= 3, fire["suppressed_label"]
    sc = int(out["short__lsp__score_cross"][gen.SHORT_CASES.index("scattered_nan_high")].sum())
    assert sc == 0, sc
    out["score_cross_scattered_sum"] = np.array(sc)
    names = sorted(drift)
    for name in names:
        n_bad, n = drift[name]
        print(f"{name}: pandas off the exact window std at {n_bad} of {n} recorded cells")
        assert n_bad < 0.005 * n, (name, n_bad, n)
    out["std_drift_columns"] = np.array(names)
    out["std_drift_cells"] = np.array([drift[k] for k in names], dtype=np.int64)
    # two files, each under the repository's 1 MiB cap on a committed file: the
    # short rows' spike columns (half the bytes) apart from everything else
    fsf = {k: v for k, v in out.items() if k.startswith("short__fsf__")}
    rest = {k: v for k, v in out.items() if k not in fsf}
    for name, arrays in (("strategy_gaps.npz", rest), ("strategy_gaps_fsf.npz", fsf)):
        np.savez_compressed(out_dir / name, **arrays)
        size = (out_dir / name).stat().st_size
        print(f"{name}: {size} bytes")
        assert size < 2**20, name


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(Path(sys.argv[2]))
        return
    if not mg.REFERENCE.exists():
        sys.exit("make_golden_strategy_gaps.py runs only where the reference is mounted")
    with tempfile.TemporaryDirectory(prefix="bq_shim_") as tmp:
        shim = Path(tmp)
        mg.write_shim(shim)
        env = dict(os.environ)
        env["PYTHONPATH"] = f"{shim}:{mg.REFERENCE}"
        env["PYTHONDONTWRITEBYTECODE"] = "1"
        env["ENV"] = "ci"
        subprocess.run([sys.executable, __file__, "--child", str(HERE)], check=True, env=env, cwd=tmp)


if __name__ == "__main__":
    main()
