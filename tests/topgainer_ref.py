"""Serial numpy / pandas restatement of bq_top_gainer_entry's contract (a test
helper: the device kernel of bq_topgainer.hip is compared with it, and it is
itself pinned to the reference by tests/golden/topgainer_gates.npz).

Column t of row s stands for TopGainerEarlyMomentum (strategies/
top_gainer_early_momentum.py) run on the frame df.iloc[first_t[s]:t + 1],
t < lens[s]: `values` / `entry` are _features (:91-159) and _entry_allows
(:161-188) of that prefix frame, `status` is signal()'s outcome (:363-406)
for the message whose newest candle is t, `score` / `stop_loss_pct` are
_score of the breakout candle t - 2 and _stop_loss_pct(close[t], atr[t])
(:236-253), both unrounded. Every point-wise value is formed with the
reference's own float64 expression (numpy's element-wise IEEE operations
round as Python's floats do); the rolling means and the ewm columns are
pandas' on the row's frame, which is causal: its value at t is the prefix
frame's last value.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

TGE_KEYS = ("close", "open", "high", "low", "volume", "quote_volume", "previous_high", "return_1h", "return_2h",
            "return_6h", "extension_return", "extension_window_bars", "extension_cap", "candle_return",
            "volume_ratio", "quote_volume_ratio", "range_position", "upper_wick_fraction", "ema20", "ema50", "atr")
TGE_REASONS = (   # code -> reason: the feature status, _entry_allows' checks in order, signal()'s own
    "top_gainer_breakout_two_close_confirmation",          # 0  :202 (entry column: top_gainer_breakout_ignition, :188)
    "history_too_short",                                   # 1  :94, :365
    "invalid_candle_values",                               # 2  :106
    "indicators_not_ready",                                # 3  :158
    "not_breaking_recent_high",                            # 4  :164
    "not_above_ema20_and_ema50",                           # 5  :166
    "candle_not_green_enough",                             # 6  :168
    "single_candle_too_extended",                          # 7  :170
    "one_hour_move_too_extended",                          # 8  :172
    "extension_move_too_extended",                         # 9  :174
    "momentum_not_accelerating",                           # 10 :179
    "six_hour_move_not_confirmed",                         # 11 :181
    "volume_ratio_too_low",                                # 12 :183
    "close_not_near_high",                                 # 13 :185
    "upper_wick_too_large",                                # 14 :187
    "first_confirmation_did_not_hold_breakout",            # 15 :199
    "second_confirmation_did_not_clear_breakout_close",    # 16 :201
    "risk_rejected",                                       # 17 :397-406
)
TGE_ENTRY_OK = "top_gainer_breakout_ignition"
FIRST_CONFIRM, SECOND_CONFIRM, RISK_REJECTED = 15, 16, 17
TGE_NO_FRAME = 255
# ema20 / ema50, the two volume ratios and score are compared at tests/util's 1e-9; the rest bit for bit
APPROX_KEYS = ("ema20", "ema50", "volume_ratio", "quote_volume_ratio")
DEFAULTS = dict(lookback_high=48, volume_window=32, min_history=56, full_extension_bars=96, min_candle_return=0.01,
                max_candle_return=0.10, min_return_1h=0.05, min_return_2h=0.08, min_return_6h=0.07,
                max_return_1h=0.20, max_extension=0.50, min_short_extension_cap=0.25, min_volume_ratio=1.75,
                min_range_position=0.75, max_upper_wick=0.30, atr_stop_mult=2.2, min_stop_loss_pct=1.5,
                max_stop_loss_pct=2.0)
TG_RISK_REASONS = ("risk_profile_allows_long", "market_context_unavailable", "market_stress_too_high",
                   "market_context_short_edge", "btc_context_down", "symbol_regime_unavailable",
                   "relative_strength_vs_btc_not_positive", "symbol_atr_too_high", "symbol_transition_not_long",
                   "symbol_trend_down")


def py_min(a, b):
    """Python's min(a, b), element-wise: b only where b < a (a NaN a sticks, a NaN b is skipped)."""
    return np.where(b < a, b, a)


def py_max(a, b):
    return np.where(b > a, b, a)


def _lag(x: np.ndarray, k: int) -> np.ndarray:
    out = np.full_like(x, np.nan)
    if k < len(x):
        out[k:] = x[: len(x) - k]
    return out


def frame_features(o, h, l, c, v, qv, atr, par) -> tuple[dict[str, np.ndarray], np.ndarray]:
    """_features at every prefix of ONE frame (arrays [n], the frame's own
    rows): (the 21 values before masking, the feature status 0 / 1 / 2 / 3)."""
    n = len(c)
    L, W, FE = int(par["lookback_high"]), int(par["volume_window"]), int(par["full_extension_bars"])
    i = np.arange(n)
    with np.errstate(all="ignore"):
        # df["high"].iloc[-L - 1:-1].max(): Series.max skips NaN and keeps +-inf
        padded = np.r_[np.full(L, np.nan), h]
        prev_high = np.fmax.reduce(np.lib.stride_tricks.sliding_window_view(padded, L)[:n], axis=1)
        vma = pd.Series(v).rolling(W).mean().to_numpy()
        if qv is not None:
            quote, qvma = qv, pd.Series(qv).rolling(W).mean().to_numpy()
        else:
            quote, qvma = v * c, vma * c
        a = np.zeros(n) if atr is None else atr
        rng = h - l
        wick = h - py_max(o, c)
        bars_i = np.minimum(i, FE)
        bars = bars_i.astype(np.float64)
        cap = np.where(bars_i < FE, py_max(np.full(n, float(par["min_short_extension_cap"])),
                                            float(par["max_extension"]) * (bars / FE)), float(par["max_extension"]))
        values = {
            "close": c, "open": o, "high": h, "low": l, "volume": v, "quote_volume": quote,
            "previous_high": prev_high,
            "return_1h": c / _lag(c, 4) - 1, "return_2h": c / _lag(c, 8) - 1, "return_6h": c / _lag(c, 24) - 1,
            "extension_return": c / c[np.maximum(i - FE, 0)] - 1,
            "extension_window_bars": bars, "extension_cap": cap,
            "candle_return": c / o - 1,
            "volume_ratio": v / (vma + 1e-6), "quote_volume_ratio": quote / (qvma + 1e-6),
            "range_position": (c - l) / (rng + 1e-6), "upper_wick_fraction": wick / (rng + 1e-6),
            "ema20": pd.Series(c).ewm(span=20, adjust=False).mean().to_numpy(),
            "ema50": pd.Series(c).ewm(span=50, adjust=False).mean().to_numpy(),
            "atr": a,
        }
        m = c
        for x in (o, h, l, v):
            m = py_min(m, x)
        finite = np.ones(n, bool)
        for k in TGE_KEYS:
            finite &= np.isfinite(values[k])
        fs = np.where(i + 1 < int(par["min_history"]), 1, np.where(m <= 0, 2, np.where(finite, 0, 3)))
    return values, fs.astype(np.uint8)


def entry_codes(values, fs, par) -> np.ndarray:
    """The feature status, else _entry_allows' first failing check, else 0."""
    x = values
    with np.errstate(all="ignore"):
        checks = [
            x["close"] <= x["previous_high"],
            (x["close"] <= x["ema20"]) | (x["close"] <= x["ema50"]),
            x["candle_return"] < par["min_candle_return"],
            x["candle_return"] > par["max_candle_return"],
            x["return_1h"] > par["max_return_1h"],
            x["extension_return"] > x["extension_cap"],
            (x["return_1h"] < par["min_return_1h"]) & (x["return_2h"] < par["min_return_2h"]),
            x["return_6h"] < par["min_return_6h"],
            x["volume_ratio"] < par["min_volume_ratio"],
            x["range_position"] < par["min_range_position"],
            x["upper_wick_fraction"] > par["max_upper_wick"],
        ]
    code = np.zeros(len(fs), np.uint8)
    for j in range(len(checks), 0, -1):
        code = np.where(checks[j - 1], j + 3, code)
    return np.where(fs != 0, fs, code).astype(np.uint8)


def top_gainer_entry(o, h, l, c, v, qv=None, atr=None, *, risk_ok=None, first_t=None, lens=None, raw=False,
                     **thresholds):
    """{"status", "entry" uint8 [S, T], "score", "stop_loss_pct" [S, T],
    "values": {key: [S, T]}} — bq_top_gainer_entry's outputs. raw=True keeps
    the values where the feature status is not ready (the near-tie checks)."""
    par = {**DEFAULTS, **thresholds}
    S, T = c.shape
    first = np.zeros(S, np.int64) if first_t is None else np.clip(np.asarray(first_t, np.int64), 0, T)
    ln = np.full(S, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    t_idx = np.arange(T)
    entry = np.where(t_idx[None, :] < ln[:, None], 1, TGE_NO_FRAME).astype(np.uint8)
    status = entry.copy()
    score, stop = np.full((S, T), np.nan), np.full((S, T), np.nan)
    out = {k: np.full((S, T), np.nan) for k in TGE_KEYS}
    for s in range(S):
        f, n = int(first[s]), int(ln[s])
        if n <= f:
            continue
        sl = slice(f, n)
        fr = [x[s, sl].astype(np.float64) for x in (o, h, l, c, v)]
        q = None if qv is None else qv[s, sl].astype(np.float64)
        a = None if atr is None else atr[s, sl].astype(np.float64)
        values, fs = frame_features(*fr, q, a, par)
        en = entry_codes(values, fs, par)
        entry[s, sl] = en
        for k in TGE_KEYS:
            out[k][s, sl] = values[k] if raw else np.where(fs == 0, values[k], np.nan)
        cc = fr[3]
        m = n - f
        i = np.arange(m)
        with np.errstate(all="ignore"):
            e2 = np.r_[np.ones(2, np.uint8), en[:-2]][:m]
            ph2, c2, c1 = _lag(values["previous_high"], 2), _lag(cc, 2), _lag(cc, 1)
            rk = np.ones(m, bool) if risk_ok is None else np.asarray(risk_ok[s, sl], bool)
            st = np.where(~rk, RISK_REJECTED, 0)
            st = np.where(cc <= c2, SECOND_CONFIRM, st)
            st = np.where(c1 <= ph2, FIRST_CONFIRM, st)
            st = np.where(e2 != 0, e2, st)
            st = np.where(i + 1 < int(par["min_history"]) + 2, 1, st)
            status[s, sl] = st
            # _score of the breakout candle, _stop_loss_pct of the candidate: unrounded
            sc = ((1.0 + py_min(values["return_1h"] * 4, np.full(m, 0.8)))
                  + py_min(values["volume_ratio"] / 10, np.full(m, 0.5))) \
                + py_min(values["range_position"] / 4, np.full(m, 0.25))
            av = values["atr"]
            pct = (par["atr_stop_mult"] * av / cc) * 100
            lo, hi = np.full(m, float(par["min_stop_loss_pct"])), np.full(m, float(par["max_stop_loss_pct"]))
            slp = np.where((cc <= 0) | (av <= 0), lo, py_min(py_max(pct, lo), hi))
            cand = (st == 0) | (st == RISK_REJECTED)
            score[s, sl] = np.where(cand, _lag(sc, 2), np.nan)
            stop[s, sl] = np.where(cand, slp, np.nan)
    return {"status": status, "entry": entry, "score": score, "stop_loss_pct": stop, "values": out}


def risk_allows(case: dict) -> int:
    """TG_RISK_REASONS' index for one stand-in context / features case (the
    keys of topgainer_panel_gen.risk_cases): _risk_profile_allows (:204-234)."""
    if not case["context_ok"]:
        return 1
    if case["stress"] >= 0.25:
        return 2
    if case["short_score"] > case["long_score"] + 0.15:
        return 3
    if case["regime_score"] < -0.2 and case["btc_return"] < 0:
        return 4
    if not case["features_ok"]:
        return 5
    if case["rs"] <= 0.03:
        return 6
    if case["atr_pct"] > 0.06:
        return 7
    if case["transition"] in ("BREAKDOWN", "ENTERED_TREND_DOWN", "VOLATILITY_EXPANSION"):
        return 8
    if case["regime"] == "TREND_DOWN" and case["trend"] < 0:
        return 9
    return 0
