"""Plain numpy restatement of two reference methods at every prefix frame
(a test helper: the device kernels of bq_impulse.hip are compared with it,
and it is itself pinned to the reference by tests/golden/impulse_gates.npz).

* impulse_rider      RelativeStrengthImpulseRider._features
                     (strategies/relative_strength_impulse_rider.py:92-198) with
                     _btc_return_at (:69-90)
* bb_stable          LadderDeployer._bb_stable (strategies/grid/ladder_deployer.py:42-56)

Column t of row s is the method on df.iloc[first_t[s]:t + 1]. Every value is
formed with the reference's own float64 expression (numpy's element-wise
IEEE operations round as Python's floats do), so the comparison is bit for
bit.
"""

from __future__ import annotations

import numpy as np

IR_KEYS = ("impulse_return_1h", "previous_impulse_return_1h", "btc_return_1h", "relative_strength_1h",
           "trigger_return_15m", "confirmation_return_15m", "confirmation_close_location", "atr_pct",
           "entry_limit_price")
IR_REASONS = (   # code -> reason, in the method's order of checks
    "relative_strength_impulse_confirmed",       # 0  :197
    "history_too_short",                         # 1  :99
    "invalid_candle_values",                     # 2  :124
    "invalid_return_anchors",                    # 3  :130
    "btc_return_unavailable",                    # 4  :137
    "confirmation_range_invalid",                # 5  :144
    "indicators_not_ready",                      # 6  :159
    "impulse_outside_range",                     # 7  :161
    "impulse_did_not_cross_threshold",           # 8  :165
    "btc_return_too_high",                       # 9  :167
    "relative_strength_too_low",                 # 10 :169
    "atr_pct_too_high",                          # 11 :171
    "confirmation_did_not_hold_trigger_close",   # 12 :173
    "confirmation_return_negative",              # 13 :175
    "confirmation_close_not_near_high",          # 14 :177
)
IR_NO_FRAME = 255
DEFAULTS = dict(min_history=20, min_impulse=0.05, max_impulse=0.18, min_rs=0.08, max_btc_return=0.01,
                min_conf_return=0.0, min_close_location=0.70, max_atr_pct=0.06, entry_factor=1 - 1.0 / 100)
# The thresholds wide open (MIN_* = -inf, MAX_* = +inf). MIN_IMPULSE_RETURN_1H serves two checks — "MIN <=
# impulse" (:161) and "previous_impulse >= MIN" rejects (:165) — so at -inf check 8 rejects every candle that
# passed checks 1-6; values are returned only where previous < MIN <= impulse. The fixture therefore records
# the wide-open thresholds once with MIN = -inf (pins checks 1-6 at every candle) and once per value of a
# small grid of MIN (pins the nine values wherever a grid point separates the two returns).
WIDE_OPEN = dict(min_impulse=-np.inf, max_impulse=np.inf, min_rs=-np.inf, max_btc_return=np.inf,
                 min_conf_return=-np.inf, min_close_location=-np.inf, max_atr_pct=np.inf)


def _shift(x: np.ndarray, k: int, fill) -> np.ndarray:
    """x[:, t - k] at column t (fill where t < k)."""
    out = np.full_like(x, fill)
    if k < x.shape[1]:
        out[:, k:] = x[:, : x.shape[1] - k]
    return out


def btc_return_at_keys(keys: np.ndarray, bench_ts: np.ndarray, bench_close: np.ndarray):
    """_btc_return_at (:69-90) for an array of open times: (return, available)."""
    bench_ts = np.asarray(bench_ts, np.int64).reshape(-1)
    bench_close = np.asarray(bench_close, np.float64).reshape(-1)
    nb = bench_ts.size
    ret = np.full(keys.shape, np.nan)
    if nb < 5:                                                       # :71
        return ret, np.zeros(keys.shape, bool)
    pos = np.searchsorted(bench_ts, keys, side="right") - 1          # the last row with this time (:74-81)
    hit = (pos >= 0) & (bench_ts[np.clip(pos, 0, nb - 1)] == keys)
    ok = hit & (pos >= 4)                                            # :82
    p = np.where(ok, pos, 4)
    anchor, close = bench_close[p - 4], bench_close[p]               # positional (:85-86)
    with np.errstate(all="ignore"):
        ok &= ~((anchor <= 0) | (close <= 0))                        # :87 (a NaN passes)
        r = close / anchor - 1                                       # :89
    ok &= np.isfinite(r)                                             # :90
    return np.where(ok, r, np.nan), ok


def impulse_rider(o, h, l, c, atr, open_time, bench_ts, bench_close, first_t=None, lens=None, raw=False,
                  **thresholds):
    """(values {key: [S, T]}, status uint8 [S, T]) at every prefix."""
    P = {**DEFAULTS, **thresholds}
    o, h, l, c, atr = (np.asarray(x, np.float64) for x in (o, h, l, c, atr))
    ts = np.asarray(open_time, np.int64)
    S, T = c.shape
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t, np.int64).reshape(S)
    ln = np.full(S, T, np.int64) if lens is None else np.asarray(lens, np.int64).reshape(S)
    t = np.arange(T)[None, :]
    nan = np.nan
    c_cf, o_cf, h_cf, l_cf = c, o, h, l                                        # confirmation = candle t (:105)
    c_tr, o_tr, a_tr = _shift(c, 1, nan), _shift(o, 1, nan), _shift(atr, 1, nan)   # trigger = candle t - 1 (:104)
    a_imp, a_prev, c_pv = _shift(c, 5, nan), _shift(c, 6, nan), _shift(c, 2, nan)  # :127-129
    key = _shift(ts, 1, 0)
    btc, btc_ok = btc_return_at_keys(key, bench_ts, bench_close)
    btc_ok &= t >= 1
    with np.errstate(all="ignore"):
        impulse = c_tr / a_imp - 1                                             # :133
        previous = c_pv / a_prev - 1                                           # :134
        rs = impulse - btc                                                     # :140
        atr_pct = a_tr / c_tr                                                  # :141
        conf_ret = c_cf / o_cf - 1                                             # :142
        rng = h_cf - l_cf                                                      # :143
        location = (c_cf - l_cf) / rng                                         # :146-148
        trig_ret = c_tr / o_tr - 1                                             # :191
        entry = c_cf * P["entry_factor"]                                       # :180
        good = np.ones((S, T), bool)
        for x in (c_tr, o_tr, o_cf, h_cf, l_cf, c_cf, a_tr):                   # :124
            good &= np.isfinite(x) & (x > 0)
        checks = [                                                             # the failing conditions, in order
            t + 1 - first[:, None] < P["min_history"],                         # 1
            ~good,                                                             # 2
            (a_imp <= 0) | (a_prev <= 0) | (c_pv <= 0),                        # 3
            ~btc_ok,                                                           # 4
            rng <= 0,                                                          # 5
            ~(np.isfinite(impulse) & np.isfinite(previous) & np.isfinite(btc) & np.isfinite(rs)
              & np.isfinite(atr_pct) & np.isfinite(conf_ret) & np.isfinite(location)),   # 6
            ~((P["min_impulse"] <= impulse) & (impulse <= P["max_impulse"])),  # 7
            previous >= P["min_impulse"],                                      # 8
            btc > P["max_btc_return"],                                         # 9
            rs < P["min_rs"],                                                  # 10
            atr_pct > P["max_atr_pct"],                                        # 11
            c_cf < c_tr,                                                       # 12
            conf_ret < P["min_conf_return"],                                   # 13
            location < P["min_close_location"],                                # 14
        ]
    status = np.zeros((S, T), np.uint8)
    for code in range(len(checks), 0, -1):
        status[checks[code - 1]] = code
    status[t >= ln[:, None]] = IR_NO_FRAME
    ok = status == 0
    cols = (impulse, previous, btc, rs, trig_ret, conf_ret, location, atr_pct, entry)
    if raw:   # the unmasked expressions (the fixture generator's near-tie check)
        return dict(zip(IR_KEYS, cols)), status
    return {k: np.where(ok, v, np.nan) for k, v in zip(IR_KEYS, cols)}, status


def bb_stable(bb_upper, bb_mid, bb_lower, n: int = 8, max_change_pct: float = 20.0, first_t=None, lens=None):
    """(stable bool [S, T], change_pct [S, T]; NaN where the method returns
    before computing it) at every prefix."""
    up, md, lw = (np.asarray(x, np.float64) for x in (bb_upper, bb_mid, bb_lower))
    S, T = md.shape
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t, np.int64).reshape(S)
    ln = np.full(S, T, np.int64) if lens is None else np.asarray(lens, np.int64).reshape(S)
    t = np.arange(T)[None, :]
    with np.errstate(all="ignore"):
        w = (up - lw) / md                                                     # :51
        bad = (md <= 0) | (w <= 0)                                             # :49, :52 (NaN passes both)
        cs = np.concatenate([np.zeros((S, 1), np.int64), np.cumsum(bad, axis=1)], axis=1)
        lo = np.clip(t - (n - 1), 0, None)
        nbad = cs[:, 1:] - np.take_along_axis(cs, np.broadcast_to(lo, (S, T)), axis=1)
        reached = (t + 1 - first[:, None] >= n) & (nbad == 0) & (t < ln[:, None])   # :44
        w0 = np.take_along_axis(w, np.broadcast_to(lo, (S, T)), axis=1)
        change = np.abs((w - w0) / w0) * 100                                   # :55
        stable = reached & (change <= max_change_pct)                          # :56
    return stable, np.where(reached, change, np.nan)
