"""Deterministic inputs of the per-frame failed-spike fixture
(tests/golden/spikeframes.npz).

Shared by tests/golden/make_golden_spikeframes.py (which runs a FRESH
FailedSpikeFade on every frame df.iloc[first:t + 1] of these rows where the
reference is mounted) and the tests (which regenerate the same inputs and
compare with the recorded outputs). Only numpy's default_rng is used; the
fixture stores a digest of the inputs.

The panel: 10 rows x 288 15-minute candles (three days). By row:

  0  quiet walk (sigma 0.2 %), a spike every 9-30 bars;
  1  dense stretches of 160 bars (a bullish +2-5 % candle on 2.5-5x volume
  2  every 4-6 bars), sparse spikes, some of them bearish, between them;
  3  high-noise walks (sigma 3 %): q75(|pct change|) exceeds the 0.03 floor;
  4
  5  as row 1, the frame starting at candle 37 (first_t > 0, not a multiple
     of 64);
  6  as row 0, 201 candles (lens < T);
  7  9 candles after first_t = 100: every frame is shorter than base_window;
  8  as row 1 with 5 % of the candles missing (close and volume together);
  9  volumes within a few percent of each other for 110 candles (q97 of the
     volume ratio stays below the 1.15 floor), then zero-volume stretches."""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 10, 288, 20261121
T0, STEP = 1_760_400_000_000, 900_000
FIRST_T = {5: 37, 7: 100}
LENS = {6: 201, 7: 109}
DENSE_ROWS = (1, 2, 5, 8)
NOISY_ROWS = (3, 4)
NAN_ROW, FLAT_ROW = 8, 9


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
        vol = g.lognormal(3.0, 0.03 if s == FLAT_ROW else 0.3, T)
        phase = int(g.integers(0, 2))
        t = int(first[s]) + 14 + int(g.integers(0, 6))
        while t < T - 1:
            dense = s in DENSE_ROWS and ((t - int(first[s])) // 160 + phase) % 2 == 0
            if not (s == FLAT_ROW and t < 110):
                r[t] = g.uniform(0.02, 0.05)
                vol[t] *= g.uniform(2.5, 5.0)
                if not dense and g.random() < 0.3:   # a bearish spike: the short side's labels
                    r[t] = -r[t]
            t += int(g.integers(4, 7)) if dense else int(g.integers(9, 30))
        if s == FLAT_ROW:
            for b in (120, 170, 230):
                vol[b:b + int(g.integers(5, 20))] = 0.0
        cc = scale * np.exp(np.cumsum(r))
        oo = np.r_[cc[0], cc[:-1]]
        hh = np.maximum(oo, cc) * (1.0 + g.uniform(0.0, 0.003, T))
        ll = np.minimum(oo, cc) * (1.0 - g.uniform(0.0, 0.003, T))
        qq = vol * cc
        if s == NAN_ROW:
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
