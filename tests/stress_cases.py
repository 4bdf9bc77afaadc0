"""Stress rows for the indicator hot path: trends, crashes, tick-size prices.

Deterministic numpy. synth.numpy_panel is a sigma = 0.002 walk around one
scale per row; the rows here do what klines do and that generator never does:
they trend for the whole row (windows all gain / all loss), gap by x0.1 ..
x100 in one candle, sit on a tick grid (values repeat, windows are constant),
and change volume regime by 1e4. Every family is ONE row; T = 2300 gives
tile 0, one interior 1024-candle tile and a tail tile.

open / high / low follow synth.numpy_symbol (open = previous close, wicks
U(0, 0.003)); a candle whose close repeats the previous close is flat
(open = high = low = close), as numpy_symbol(edges=True) builds it.

Each Family carries its event candles (where a step, pump or regime change
happens), its exact plateaus [a, b) and its zero-volume runs [a, b).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

FIELDS = ("open", "high", "low", "close", "volume")
T_DEFAULT = 2300
PLATEAUS = ((200, 240), (1010, 1130), (2040, 2060))
ZERO_VOLUME = ((300, 330), (1015, 1045))


@dataclass
class Family:
    name: str
    open: np.ndarray
    high: np.ndarray
    low: np.ndarray
    close: np.ndarray
    volume: np.ndarray
    events: tuple = ()
    plateaus: tuple = ()
    zero_volume: tuple = ()
    meta: dict = field(default_factory=dict)


def _seed(name: str) -> int:
    return int.from_bytes(name.encode(), "little") % (2**31 - 1)


def _candles(name, close, volume=None, events=(), plateaus=(), zero_volume=(), integer_volume=False):
    """open / high / low around a close series, numpy_symbol's way."""
    close = np.asarray(close, dtype=np.float64)
    T = close.size
    rng = np.random.default_rng(_seed(name) + 1)
    open_ = np.empty(T)
    open_[0] = close[0]
    open_[1:] = close[:-1]
    high = np.maximum(open_, close) * (1.0 + rng.uniform(0.0, 0.003, T))
    low = np.minimum(open_, close) * (1.0 - rng.uniform(0.0, 0.003, T))
    if volume is None:
        volume = rng.lognormal(3.0, 1.0, T)
    if integer_volume:
        volume = np.floor(volume) + 1.0
    volume = np.array(volume, dtype=np.float64)
    for a, b in zero_volume:
        volume[a:b] = 0.0
    flat = close == np.roll(close, 1)
    flat[0] = False
    open_[flat] = close[flat]
    high[flat] = close[flat]
    low[flat] = close[flat]
    for a, b in plateaus:
        assert (close[a:b] == close[a]).all() and close[a - 1] != close[a] and (b >= T or close[b] != close[a]), name
    return Family(name, open_, high, low, close, volume, tuple(events), tuple(plateaus), tuple(zero_volume))


def _walk(name, T, scale, sigma=0.002):
    rng = np.random.default_rng(_seed(name))
    return scale * np.exp(np.cumsum(rng.normal(0.0, sigma, T)))


def ramp(name, T, rate):
    return _candles(name, 100.0 * np.exp(rate * np.arange(T)))


def step(name, T, event, factor):
    """sigma = 0.002 walk around 50, multiplied by `factor` from `event` on."""
    c = _walk("step", T, 50.0)   # one walk shared by every crash / spike family
    c[event:] *= factor
    return _candles(name, c, events=(event,))


def tick2_plateau(name, T, plateaus=PLATEAUS, zero_volume=ZERO_VOLUME):
    rng = np.random.default_rng(_seed("tick2_plateau"))
    c = np.maximum(np.round(1.0 + np.cumsum(rng.normal(0.0, 0.006, T)), 2), 0.05)
    for a, b in plateaus:
        # an exact plateau whose neighbours differ from it by at least a tick
        c[a:b] = c[a]
        for j in (a - 1, b):
            if 0 <= j < T and c[j] == c[a]:
                c[j] = np.round(c[a] + 0.01, 2)
    edges = tuple(x for ab in plateaus for x in ab)
    return _candles(name, c, events=edges, plateaus=plateaus, zero_volume=zero_volume, integer_volume=True)


def pump_dump(name, T):
    rng = np.random.default_rng(_seed(name))
    ret = rng.normal(0.0, 0.002, T)
    events = []
    for s in range(150, T - 16, 150):
        ret[s : s + 10] = np.log(1.35)
        ret[s + 10 : s + 16] = np.log(0.60)
        events += [s, s + 10]
    return _candles(name, 0.01 * np.exp(np.cumsum(ret)), events=events)


def micro(name, T):
    return _candles(name, np.round(_walk(name, T, 1.234e-5, sigma=0.01), 8))


def huge(name, T):
    f = _candles(name, _walk(name, T, 3e9))
    f.volume = f.volume * 1e10
    return f


def zigzag(name, T):
    return _candles(name, np.where(np.arange(T) % 2 == 0, 100.00, 100.01))


def tight_high(name, T):
    rng = np.random.default_rng(_seed(name))
    return _candles(name, np.round(60000.0 + rng.normal(0.0, 0.5, T), 1))


def vol_drop(name, T, event=600, factor=1e4):
    f = _candles(name, _walk(name, T, 50.0), events=(event,), zero_volume=ZERO_VOLUME)
    f.volume[:event] *= factor
    return f


def families(T: int = T_DEFAULT) -> list[Family]:
    out = [ramp("ramp_up", T, 0.005), ramp("ramp_down", T, -0.005), tick2_plateau("tick2_plateau", T)]
    out += [step(f"crash10@{e}", T, e, 0.1) for e in (700, 1024, 2048)]
    out += [step(f"spike10@{e}", T, e, 10.0) for e in (700, 1024, 2048)]
    out += [step("crash100@1024", T, 1024, 0.01), step("spike100@1024", T, 1024, 100.0)]
    out += [pump_dump("pump_dump", T), micro("micro", T), huge("huge", T), zigzag("zigzag", T),
            tight_high("tight_high", T), vol_drop("vol_drop_1e4", T)]
    return out


def long_families(T: int = 4100) -> list[Family]:
    """The carry of the 2048-candle tiles of bq_wilder_rsi / bq_adx /
    bq_zscore: the crash and a plateau across candle 2048, with a full tile
    and a tail after it."""
    return [step("crash10@2048", T, 2048, 0.1), tick2_plateau("tick2_plateau", T)]


def panel(fams: list[Family]) -> dict[str, np.ndarray]:
    return {k: np.stack([getattr(f, k) for f in fams]) for k in FIELDS}


def names(fams: list[Family]) -> list[str]:
    return [f.name for f in fams]
