"""Deterministic inputs of the capped per-frame failed-spike fixture
(tests/golden/spikecap.npz).

Shared by tests/golden/make_golden_spikecap.py (which runs a FRESH
FailedSpikeFade on every capped frame df.iloc[max(first, t + 1 - M):t + 1] of
these rows where the reference is mounted) and the tests (which regenerate the
same inputs and compare with the recorded outputs). Only numpy's default_rng
is used; the fixture stores a digest of the inputs.

The panel: 8 rows x 420 15-minute candles, so that a cap of 301 rows (the live
store's LIMIT = 400 less the warm-up rows post_process drops) bites. By row:

  0  dense stretches of 200 bars (a bullish +2-5 % candle on 2.5-5x volume
  1  every 4-6 bars), sparse spikes, some of them bearish, between them;
     row 1's frame starts at candle 37 (first_t > 0, not a multiple of 64);
  2  high-noise walk (sigma 3 %): q75(|pct change|) exceeds the 0.03 floor;
  3  as row 0 with 5 % of the candles missing (close and volume together);
  4  quiet walk (sigma 0.2 %), a spike every 9-30 bars, 333 candles (lens < T);
  5  as row 3, the frame starting at candle 21;
  6  as row 2 with 5 % of the candles missing: a frame that starts on a
     missing close loses observations that move the raised price floor;
  7  as row 0, the other phase of the stretches."""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 8, 420, 20261021
CAPS = (64, 96, 301)
T0, STEP = 1_760_400_000_000, 900_000
FIRST_T = {1: 37, 5: 21}
LENS = {4: 333}
DENSE_ROWS = (0, 1, 3, 5, 7)
NOISY_ROWS = (2, 6)
NAN_ROWS = (3, 5, 6)
STRETCH = 200


def frames_panel(seed: int = SEED) -> dict[str, np.ndarray]:
    cols = {k: np.full((S, T), np.nan) for k in ("open", "high", "low", "close", "volume", "quote_asset_volume")}
    lens = np.full(S, T, np.int64)
    first = np.zeros(S, np.int64)
    for s, f in FIRST_T.items():
        first[s] = f
    for s, n in LENS.items():
        lens[s] = n
    for s in range(S):
        g = np.random.default_rng(seed * 1000 + s)
        scale = 10.0 ** g.uniform(-1.0, 3.0)
        r = g.normal(0.0, 0.03 if s in NOISY_ROWS else 0.002, T)
        vol = g.lognormal(3.0, 0.3, T)
        phase = 1 if s == 7 else int(g.integers(0, 2))
        t = int(first[s]) + 14 + int(g.integers(0, 6))
        while t < T - 1:
            dense = s in DENSE_ROWS and ((t - int(first[s])) // STRETCH + phase) % 2 == 0
            r[t] = g.uniform(0.02, 0.05)
            vol[t] *= g.uniform(2.5, 5.0)
            if not dense and g.random() < 0.3:   # a bearish spike: the short side's labels
                r[t] = -r[t]
            t += int(g.integers(4, 7)) if dense else int(g.integers(9, 30))
        cc = scale * np.exp(np.cumsum(r))
        oo = np.r_[cc[0], cc[:-1]]
        hh = np.maximum(oo, cc) * (1.0 + g.uniform(0.0, 0.003, T))
        ll = np.minimum(oo, cc) * (1.0 - g.uniform(0.0, 0.003, T))
        qq = vol * cc
        if s in NAN_ROWS:
            hole = g.random(T) < 0.05
            cc, vol, qq = (np.where(hole, np.nan, x) for x in (cc, vol, qq))
        n = int(lens[s])
        for k, v in (("open", oo), ("high", hh), ("low", ll), ("close", cc), ("volume", vol),
                     ("quote_asset_volume", qq)):
            cols[k][s, :n] = v[:n]
    ts = T0 + STEP * np.arange(T, dtype=np.int64)[None, :] + np.zeros((S, 1), np.int64)
    return dict(**cols, open_time=ts, lens=lens, first_t=first)


def digest(panel: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for f in sorted(panel):
        h.update(f.encode())
        h.update(np.ascontiguousarray(panel[f]).tobytes())
    return h.hexdigest()
