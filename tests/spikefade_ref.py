"""Plain serial numpy restatement of FailedSpikeFade.signal()'s pending-spike
state machine (strategies/failed_spike_fade.py:596-695) and of its allow
helpers (:155-203), pinned to the REAL methods by tests/golden/spikefade_gates.npz
(tests/test_spikefade_ref.py) and used as the oracle of the device kernel
(bq_spike_fade_replay) at shapes the fixture does not hold.

One candle at a time, one row at a time, Python floats: every test is the
method's own expression (at most one multiply, one compare, in its direction)."""

from __future__ import annotations

import numpy as np

(FS_IDLE, FS_SOURCE_SET, FS_WAITING, FS_CANDIDATE, FS_CLEARED, FS_SAME_CANDLE) = range(6)
FS_NO_FRAME = 255
FS_EVENTS = ("idle", "source_set", "waiting", "candidate", "cleared", "same_candle")
D_SOURCE, D_MARKET, D_NEW_HIGH, D_CANDLE_EXPIRED, D_WINDOW_EXPIRED, D_EXTENSION = 1, 2, 4, 8, 16, 32

DEFAULTS = dict(window_bars=8, ext_factor=1 + 0.06)
MAX_WINDOW = 32
BARS_MAX = 255   # the bars column is a byte: a carried-in spike found further back saturates


def nanmax_or_nan(x: np.ndarray) -> float:
    """pandas' Series.max(): NaN skipped, NaN only if all are NaN (or none)."""
    x = x[~np.isnan(x)]
    return float(x.max()) if len(x) else float("nan")


def _mask(m, s, t):
    if m is None:
        return True
    m = np.asarray(m)
    return bool(m[t] if m.ndim == 1 else m[s, t])


def spike_fade_replay(o, h, c, open_time, source_ok, src_market=None, fail_market=None, *, first_t=None, lens=None,
                      from_t=None, state=None, trace=False, **params):
    """Returns (event uint8 [S, T], detail uint8 [S, T], bars uint8 [S, T],
    state) with state = (active bool [S], open_time int64 [S], high [S],
    close [S]) after each row's last replayed candle (0 / NaN where idle).
    src_market / fail_market: [S, T] or [T] (shared by all rows) or None
    (allowed). `state`: the carried-in four (not modified; None: idle).
    trace=True adds a fifth value: the state after EVERY candle."""
    bad = set(params) - set(DEFAULTS)
    assert not bad, bad
    P = {**DEFAULTS, **params}
    W, ef = int(P["window_bars"]), float(P["ext_factor"])
    assert 1 <= W <= MAX_WINDOW and np.isfinite(ef)
    S, T = c.shape
    ev = np.full((S, T), FS_NO_FRAME, np.uint8)
    dt = np.zeros((S, T), np.uint8)
    br = np.zeros((S, T), np.uint8)
    act = np.zeros(S, bool) if state is None else np.array(state[0], bool)
    sot = np.zeros(S, np.int64) if state is None else np.array(state[1], np.int64)
    shi = np.full(S, np.nan) if state is None else np.array(state[2], np.float64)
    scl = np.full(S, np.nan) if state is None else np.array(state[3], np.float64)
    tr = (np.zeros((S, T), bool), np.zeros((S, T), np.int64), np.full((S, T), np.nan), np.full((S, T), np.nan))
    for s in range(S):
        first = 0 if first_t is None else min(max(int(first_t[s]), 0), T)
        n = T if lens is None else min(max(int(lens[s]), 0), T)
        f = max(0 if from_t is None else min(max(int(from_t[s]), 0), T), first)   # before first: an empty frame
        active, p_ot, p_hi, p_cl = bool(act[s]), int(sot[s]), float(shi[s]), float(scl[s])
        if not active:
            p_ot, p_hi, p_cl = 0, float("nan"), float("nan")
        for t in range(T):
            if f <= t < n:
                if not active:   # :618-646
                    a, m = bool(source_ok[s, t]), _mask(src_market, s, t)
                    if a and m:
                        active, p_ot, p_hi, p_cl = True, int(open_time[s, t]), float(h[s, t]), float(c[s, t])
                        ev[s, t] = FS_SOURCE_SET
                    else:
                        ev[s, t] = FS_IDLE
                        dt[s, t] = (0 if a else D_SOURCE) | (0 if m else D_MARKET)
                else:
                    pos = np.flatnonzero(open_time[s, first:t + 1] == p_ot)
                    cleared = 0
                    if len(pos) == 0:   # :652-655
                        cleared = D_CANDLE_EXPIRED
                    else:
                        p = first + int(pos[-1])
                        bars = t - p
                        if bars <= 0:   # :660-661
                            ev[s, t] = FS_SAME_CANDLE
                        else:
                            br[s, t] = min(bars, BARS_MAX)
                            if bars > W:   # :662-665
                                cleared = D_WINDOW_EXPIRED
                            elif nanmax_or_nan(np.asarray(h[s, p + 1:t + 1], np.float64)) > p_hi * ef:   # :667-677
                                cleared = D_EXTENSION
                            else:
                                fnh = float(h[s, t]) >= p_hi and float(c[s, t]) < float(o[s, t]) \
                                    and float(c[s, t]) < p_cl
                                m = _mask(fail_market, s, t)
                                if not fnh or not m:   # :685-693
                                    ev[s, t] = FS_WAITING
                                    dt[s, t] = (0 if fnh else D_NEW_HIGH) | (0 if m else D_MARKET)
                                else:   # :695
                                    ev[s, t] = FS_CANDIDATE
                                    active = False
                    if cleared:
                        ev[s, t], dt[s, t] = FS_CLEARED, cleared
                        active = False
                    if not active:
                        p_ot, p_hi, p_cl = 0, float("nan"), float("nan")
            tr[0][s, t], tr[1][s, t], tr[2][s, t], tr[3][s, t] = active, p_ot, p_hi, p_cl
        act[s], sot[s], shi[s], scl[s] = active, p_ot, p_hi, p_cl
    out = (ev, dt, br, (act, sot, shi, scl))
    return out + (tr,) if trace else out


# FailedSpikeFade.source_spike_allows' reasons (:190-203): index 0 allows, then the first failing check
SPIKE_SOURCE_REASONS = ("symbol_confirmed_upward_price_impulse", "symbol_price_impulse_missing",
                        "symbol_spike_too_extended", "symbol_upward_spike_missing")
# source_market_allows / failure_market_allows' reasons (:155-188): indices 0 and 1 allow (the reference
# appends the breadth series' key to them), then the first failing check
SPIKE_MARKET_REASONS = ("source_breadth_up", "failure_breadth_down", "market_context_unavailable",
                        "market_stress_too_high", "market_context_not_long", "breadth_momentum_unavailable",
                        "source_breadth_not_up", "failure_breadth_not_down")


def market_reason_code(reason: str) -> int:
    for i, r in enumerate(SPIKE_MARKET_REASONS):
        if reason == r or (i < 2 and reason.startswith(r + "_")):
            return i
    raise KeyError(reason)


def spike_source_allows(label, price_break, cum_break, accel, close_open_ratio, upward, max_candle_return=0.06):
    """Element-wise (ok, reason code); a NaN ratio passes (nan > x is False)."""
    label, pb, cb, ac, up = (np.asarray(x).astype(bool) for x in (label, price_break, cum_break, accel, upward))
    cor = np.asarray(close_open_ratio, np.float64)
    reason = np.where(~label | ~(pb | cb | ac), 1, np.where(cor > max_candle_return, 2, np.where(up, 0, 3)))
    return reason == 0, reason.astype(np.uint8)


def spike_fade_market_allows(stress, long_score, short_score, context_ok, momentum, max_market_stress=0.35,
                             min_momentum=0.5):
    """Element-wise (source_ok, source_reason, failure_ok, failure_reason); a
    NaN momentum is breadth_momentum_unavailable."""
    stress, lo, sh, mom = (np.asarray(x, np.float64) for x in (stress, long_score, short_score, momentum))
    ctx = np.asarray(context_ok).astype(bool)
    src = np.where(~ctx, 2, np.where(stress >= max_market_stress, 3, np.where(lo <= sh, 4, np.where(
        np.isnan(mom), 5, np.where(mom >= min_momentum, 0, 6)))))
    fail = np.where(~ctx, 2, np.where(stress >= max_market_stress, 3, np.where(
        np.isnan(mom), 5, np.where(mom <= -min_momentum, 1, 7))))
    return src == 0, src.astype(np.uint8), fail == 1, fail.astype(np.uint8)
