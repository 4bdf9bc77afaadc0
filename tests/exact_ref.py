"""Plain long-double reference of the indicator columns and signal helpers.

The definitions are those of oracle/indicators_ref.py (the 14 enrich
columns), of signals.wilder_rsi and of RangeBbRsiMeanReversion._compute_adx /
_compute_zscore (the formulas recorded by tests/golden/make_golden.py),
restated without any running state: every window is summed directly from its
own elements (sliding_window_view), the variance is two-pass, the EMAs are the
plain recursion y = (1 - a) y + a x seeded with x[0]. pandas' online rolling
sums lose digits after a crash or along a ramp; this reference does not, so a
kernel can be held to the value itself (tests/stress_bar.py).

All inputs are [S, T] float64 panels without missing candles; all outputs are
[S, T] np.longdouble.
"""

from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, (
    f"tests/exact_ref.py needs an extended long double (>= 63 mantissa bits), this platform's has "
    f"{np.finfo(LD).nmant}: it would be no more exact than the float64 code under test"
)

DEFAULTS = dict(ma_periods=(7, 25, 100), macd_fast=12, macd_slow=26, macd_signal=9, rsi_window=14, bb_window=20,
                bb_ddof=1, bb_k=2.0, atr_window=14, twap_window=12, ema_spans=(20, 50), mfi_window=14)
# canonical slot names (oracle CANONICAL order); the ma / ema slots keep their
# default names under other periods, as engine.enrich's outputs do
CANONICAL = ("ma_7", "ma_25", "ma_100", "macd", "macd_signal", "rsi", "bb_upper", "bb_mid", "bb_lower", "ATR",
             "twap", "ema20", "ema50", "mfi")
NAN = LD("nan")


def _ld(x):
    x = np.asarray(x, dtype=LD)
    return x[None] if x.ndim == 1 else x


def windows(x, w: int):
    """[S, T - w + 1, w] view: the window ending at candle t is [:, t - w + 1]."""
    return sliding_window_view(x, w, axis=-1)


def window_sum(x, w: int):
    x = _ld(x)
    out = np.full(x.shape, NAN, dtype=LD)
    if x.shape[-1] >= w:
        out[:, w - 1 :] = windows(x, w).sum(axis=-1)
    return out


def window_mean(x, w: int):
    return window_sum(x, w) / LD(w)


def window_var(x, w: int, ddof: int):
    """Two passes: the mean of the window, then the squared deviations from it."""
    x = _ld(x)
    out = np.full(x.shape, NAN, dtype=LD)
    if x.shape[-1] >= w and w > ddof:
        win = windows(x, w)
        m = win.sum(axis=-1) / LD(w)
        d = win - m[..., None]
        out[:, w - 1 :] = (d * d).sum(axis=-1) / LD(w - ddof)
    return out


def ema(x, alpha):
    """y[0] = x[0], y[t] = (1 - alpha) y[t-1] + alpha x[t]; `alpha` a scalar or
    one per leading row of x ([K, S, T] with K alphas runs K recursions at once)."""
    x = np.asarray(x, dtype=LD)
    a = np.asarray(alpha, dtype=LD).reshape((-1,) + (1,) * (x.ndim - 2)) if np.ndim(alpha) else LD(alpha)
    out = np.empty_like(x)
    y = x[..., 0].copy()
    out[..., 0] = y
    om = LD(1) - a
    for t in range(1, x.shape[-1]):
        y = om * y + a * x[..., t]
        out[..., t] = y
    return out


def span_alpha(span: int):
    return LD(2) / LD(span + 1)


def true_range(h, l, c):
    """TR with a skip-NaN max: the first candle, without a previous close, is high - low."""
    h, l, c = _ld(h), _ld(l), _ld(c)
    prev = np.full(c.shape, NAN, dtype=LD)
    prev[:, 1:] = c[:, :-1]
    return np.fmax(np.fmax(h - l, np.abs(h - prev)), np.abs(l - prev))


def _ratio_index(pos, neg):
    """100 - 100 / (1 + pos / neg) with IEEE rules: 100 where neg == 0 < pos,
    0 where pos == 0 < neg, NaN where both are 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return LD(100) - LD(100) / (LD(1) + pos / neg)


def enrich(o, h, l, c, v, p: dict | None = None, with_ema: bool = True) -> dict[str, np.ndarray]:
    """The 14 columns; with_ema=False leaves out the four recursions (macd, macd_signal, ema20, ema50)."""
    p = {**DEFAULTS, **(p or {})}
    o, h, l, c, v = (_ld(x) for x in (o, h, l, c, v))
    out = {}
    for slot, period in zip(("ma_7", "ma_25", "ma_100"), p["ma_periods"]):
        out[slot] = window_mean(c, period)
    if with_ema:
        alphas = [span_alpha(s) for s in (p["macd_fast"], p["macd_slow"], *p["ema_spans"])]
        e = ema(np.broadcast_to(c, (4,) + c.shape), alphas)
        out["macd"] = e[0] - e[1]
        out["macd_signal"] = ema(out["macd"], span_alpha(p["macd_signal"]))
        out["ema20"], out["ema50"] = e[2], e[3]
    # SMA RSI: delta.where(delta > 0, 0.0): the first candle's NaN delta counts as 0
    delta = np.zeros_like(c)
    delta[:, 1:] = c[:, 1:] - c[:, :-1]
    gain = window_mean(np.where(delta > 0, delta, LD(0)), p["rsi_window"])
    loss = window_mean(np.where(delta < 0, -delta, LD(0)), p["rsi_window"])
    out["rsi"] = _ratio_index(gain, loss)
    mid = window_mean(c, p["bb_window"])
    std = np.sqrt(window_var(c, p["bb_window"], p["bb_ddof"]))
    out["bb_mid"] = mid
    out["bb_upper"] = mid + LD(p["bb_k"]) * std
    out["bb_lower"] = mid - LD(p["bb_k"]) * std
    out["ATR"] = window_mean(true_range(h, l, c), p["atr_window"])
    out["twap"] = window_mean((o + h + l + c) / LD(4), p["twap_window"])
    tp = (h + l + c) / LD(3)
    mf = tp * v
    up = np.zeros(c.shape, dtype=bool)
    dn = np.zeros(c.shape, dtype=bool)
    up[:, 1:] = tp[:, 1:] > tp[:, :-1]
    dn[:, 1:] = tp[:, 1:] < tp[:, :-1]
    pos = window_sum(np.where(up, mf, LD(0)), p["mfi_window"])
    neg = window_sum(np.where(dn, mf, LD(0)), p["mfi_window"])
    out["mfi"] = _ratio_index(pos, neg)
    return {k: out[k] for k in CANONICAL if k in out}


def wilder_rsi(c, window: int = 14):
    """ewm(alpha = 1 / window, min_periods = window, adjust=False) of the
    clipped deltas (the first delta is missing: the recursion is seeded at
    candle 1 and candle t holds t observations), 100 g / (g + l), 50 where
    g + l == 0."""
    c = _ld(c)
    S, T = c.shape
    out = np.full((S, T), NAN, dtype=LD)
    if T < 2:
        return out
    delta = c[:, 1:] - c[:, :-1]
    g = ema(np.stack([np.maximum(delta, LD(0)), np.maximum(-delta, LD(0))]), LD(1) / LD(window))
    den = g[0] + g[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den != 0, LD(100) * g[0] / den, LD(50))
    out[:, window:] = r[:, window - 1 :]
    return out


def adx(h, l, c, window: int = 14):
    """_compute_adx at every candle: +DM / -DM and TR summed over `window`,
    dx = 100 |+DI - -DI| / (+DI + -DI) with 0 where that is undefined (short
    history, a zero TR sum, a zero DI total), mean of dx over `window`; 100
    while fewer than `window` candles exist."""
    h, l, c = _ld(h), _ld(l), _ld(c)
    hd = np.zeros_like(h)
    ld_ = np.zeros_like(l)
    hd[:, 1:] = h[:, 1:] - h[:, :-1]
    ld_[:, 1:] = -(l[:, 1:] - l[:, :-1])
    plus = np.where((hd > ld_) & (hd > 0), hd, LD(0))
    minus = np.where((ld_ > hd) & (ld_ > 0), ld_, LD(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        atr_sum = window_sum(true_range(h, l, c), window)
        pdi = LD(100) * window_sum(plus, window) / atr_sum
        mdi = LD(100) * window_sum(minus, window) / atr_sum
        tot = pdi + mdi
        dx = LD(100) * np.abs(pdi - mdi) / np.where(tot != 0, tot, NAN)
    dx = np.where(np.isnan(dx), LD(0), dx)
    a = window_mean(dx, window)
    return np.where(np.isnan(a), LD(100), a)


def zscore(c, window: int = 20):
    """_compute_zscore at every candle: (c - mean) / std(ddof 0) of the last
    `window` closes; 0 where the std is 0 or the history is short."""
    c = _ld(c)
    m = window_mean(c, window)
    sd = np.sqrt(window_var(c, window, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (c - m) / sd
    return np.where((sd == 0) | np.isnan(sd), LD(0), z)


def market_features_at(h, l, c, t: int, max_bars: int, a20=None, a50=None) -> dict[str, np.ndarray]:
    """_compute_symbol_features of every row at one candle t >= 1 over the
    capped history [max(0, t - max_bars + 1), t] (oracle/market_ref
    .symbol_features): EMAs seeded at the history's first candle, ATR and
    Bollinger over the last min(14 / 20, n) candles (min_periods 1, ddof 0;
    the history's first TR is high - low)."""
    h, l, c = _ld(h), _ld(l), _ld(c)
    a20 = span_alpha(20) if a20 is None else a20
    a50 = span_alpha(50) if a50 is None else a50
    s = max(0, t - max_bars + 1)
    hw, lw, cw = h[:, s : t + 1], l[:, s : t + 1], c[:, s : t + 1]
    n = cw.shape[1]
    e = ema(np.broadcast_to(cw, (2,) + cw.shape), [a20, a50])[:, :, -1]
    tr = true_range(hw, lw, cw)[:, -min(14, n) :]
    atr = tr.sum(axis=-1) / LD(tr.shape[1])
    win = cw[:, -min(20, n) :]
    mid = win.sum(axis=-1) / LD(win.shape[1])
    d = win - mid[:, None]
    sd = np.sqrt((d * d).sum(axis=-1) / LD(win.shape[1]))
    last, prev = cw[:, -1], cw[:, -2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(
            return_pct=np.where(prev == 0, LD(0), (last - prev) / np.abs(prev)),
            ema20=e[0], ema50=e[1],
            trend_score=np.where(e[1] != 0, (e[0] - e[1]) / np.abs(e[1]), LD(0)),
            atr_pct=np.where(last != 0, atr / last, LD(0)),
            bb_width=np.where(mid != 0, ((mid + 2 * sd) - (mid - 2 * sd)) / np.abs(mid), LD(0)),
        )
