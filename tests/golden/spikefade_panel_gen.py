"""Deterministic inputs of the failed-spike-fade fixture
(tests/golden/spikefade_gates.npz).

Shared by tests/golden/make_golden_spikefade.py (which drives the REAL
FailedSpikeFade.signal() over these inputs where the reference is mounted) and
the tests (which regenerate the same inputs and compare with the recorded
outputs). Only numpy's default_rng is used; the fixture stores a digest of the
inputs, so a generator drift shows up as a digest mismatch, not as a parity
failure.

The panel: 24 rows x 200 15-minute candles, each with a per-candle market
context (stress, long / short regime scores, present or not) and a breadth
momentum series (points; NaN = unavailable). A quiet random walk carries
engineered sequences about every 22 candles: two small green candles, then a
green candle of 3.5-5.5 % on a volume multiple (detect()'s price-break label
with an upward streak: the source spike), followed by one of (KINDS):

  fade       within a few candles a red candle revisits the spike high and
             closes below the spike close while breadth momentum is down;
  blocked    the same failed new high twice while the failure market gate is
             shut, then once more with it open (blocked, then candidate);
  fade8      seven quiet candles, the failing candle at bars == 8;
  extend     a candle whose high goes 6.5-9 % beyond the spike high;
  quiet      nine quiet candles: the window expires at bars == 9;
  nofirst    the source market gate is shut on the spike candle (idle, market);
  nanfade /  as fade / quiet with missing highs inside the post-spike window.
  nanquiet

Rows FIRST_T start their frame late; rows SHORT are shorter than T (NaN
padding, ascending pad times); REPEAT_ROWS get a second message on every
source candle (the generator's business)."""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 24, 200, 20261101
T0, STEP = 1_760_400_000_000, 900_000
KINDS = ("fade", "blocked", "fade8", "extend", "quiet", "nofirst", "nanfade", "nanquiet")
FIRST_T = {20: 7, 21: 31, 22: 50, 23: 64}
SHORT = {18: 171, 19: 150}
REPEAT_ROWS = (0, 5, 11, 22)
NAN_ROWS = (3, 9, 14)   # rows whose sequences are mostly of the nan kinds


def fade_panel(seed: int = SEED) -> dict[str, np.ndarray]:
    cols = {k: np.full((S, T), np.nan) for k in ("open", "high", "low", "close", "volume", "quote_asset_volume")}
    ts = np.empty((S, T), np.int64)
    stress, lng, sht, mom = (np.empty((S, T)) for _ in range(4))
    ctx = np.ones((S, T), bool)
    kind_at = np.full((S, T), -1, np.int8)   # the sequence kind on its spike candle
    lens = np.full(S, T, np.int64)
    first = np.zeros(S, np.int64)
    for s, f in FIRST_T.items():
        first[s] = f
    for s, n in SHORT.items():
        lens[s] = n
    for s in range(S):
        g = np.random.default_rng(seed * 1000 + s)
        scale = 10.0 ** g.uniform(-2.0, 3.0)
        r = g.normal(0.0, 0.0025, T)
        up = g.uniform(0.0, 0.0030, T)
        dn = g.uniform(0.0, 0.0030, T)
        vol = g.lognormal(3.0, 0.35, T)
        # the background market: mostly open for a source, sometimes one blocker
        st = np.where(g.random(T) < 0.08, g.choice([0.35, 0.4, 0.6], T), g.choice([0.05, 0.2, 0.3499], T))
        lo = g.choice([0.55, 0.6, 0.7], T)
        sh = np.where(g.random(T) < 0.08, lo + g.choice([0.0, 0.1], T), g.choice([0.2, 0.3], T))
        mo = g.choice([0.5, 0.8, 1.7], T) * np.where(g.random(T) < 0.35, -1.0, 1.0)
        mo = np.where(g.random(T) < 0.10, g.choice([0.2, -0.3, 0.4999], T), mo)
        mo[g.random(T) < 0.05] = np.nan
        ok = g.random(T) > 0.04
        hi_over = np.full(T, np.nan)   # explicit highs, as a multiple of the spike high
        hi_nan = np.zeros(T, bool)
        spikes = []
        b = int(first[s]) + 26 + int(g.integers(0, 6))
        while b + 12 < lens[s]:
            kind = KINDS[int(g.integers(0, len(KINDS)))]
            if s in NAN_ROWS and g.random() < 0.6:
                kind = ("nanfade", "nanquiet")[int(g.integers(0, 2))]
            r[b - 2:b] = g.uniform(0.003, 0.006, 2)
            r[b] = g.uniform(0.035, 0.055)
            vol[b] *= g.uniform(3.0, 6.0)
            up[b] = g.uniform(0.002, 0.004)
            kind_at[s, b] = KINDS.index(kind)
            spikes.append(b)
            w = slice(b + 1, b + 11)
            r[w] = -np.abs(g.normal(0.0008, 0.0005, 10))   # a quiet, slightly sinking tail
            up[w] = g.uniform(0.0, 0.0004, 10)
            st[b:b + 11], ok[b:b + 11] = 0.1, True
            lo[b:b + 11], sh[b:b + 11] = 0.6, 0.3
            mo[b] = g.choice([0.5, 0.9, 1.4])
            mo[w] = g.choice([0.2, -0.3, -0.9, -1.5], 10)   # the failure gate open on about half of the tail
            fails = ()
            if kind in ("fade", "nanfade"):
                fails = (b + int(g.integers(1, 5)),)
            elif kind == "blocked":
                k = b + int(g.integers(1, 4))
                fails = (k, k + 1, k + 2)
            elif kind == "fade8":
                fails = (b + 8,)
            elif kind == "extend":
                k = b + int(g.integers(1, 8))
                hi_over[k] = g.uniform(1.065, 1.09)
                mo[k] = g.choice([-0.9, 0.3])
            elif kind == "nofirst":
                mo[b] = g.choice([0.1, 0.4999, -0.8]) if g.random() < 0.6 else np.nan
                if g.random() < 0.3:
                    st[b] = 0.35
            for i, k in enumerate(fails):
                r[k] = -g.uniform(0.004, 0.009)
                hi_over[k] = g.uniform(1.0005, 1.02)
                mo[k] = g.choice([-0.5, -0.9, -2.0])
                if kind == "blocked" and i < 2:
                    mo[k] = g.choice([0.3, -0.4999])
                    if g.random() < 0.3:
                        mo[k], st[k] = -0.9, 0.5
            if kind in ("nanfade", "nanquiet"):
                holes = b + 1 + g.choice(8, int(g.integers(1, 4)), replace=False)
                hi_nan[holes[~np.isin(holes, fails)]] = True
                if kind == "nanquiet" and g.random() < 0.5:
                    hi_nan[b + 1:b + 10] = True   # every high of the window missing
            b += 20 + int(g.integers(0, 6))
        cc = scale * np.exp(np.cumsum(r))
        oo = np.r_[cc[0], cc[:-1]]
        hh = np.maximum(oo, cc) * (1.0 + up)
        ll = np.minimum(oo, cc) * (1.0 - dn)
        for b in spikes:
            k = np.arange(b + 1, min(b + 11, T))
            sel = k[~np.isnan(hi_over[k])]
            hh[sel] = np.maximum(hh[sel], hh[b] * hi_over[sel])
        hh[hi_nan] = np.nan
        n = int(lens[s])
        for k, v in (("open", oo), ("high", hh), ("low", ll), ("close", cc), ("volume", vol),
                     ("quote_asset_volume", vol * cc)):
            cols[k][s, :n] = v[:n]
        ts[s] = T0 + STEP * np.arange(T, dtype=np.int64)
        stress[s], lng[s], sht[s], mom[s], ctx[s] = st, lo, sh, mo, ok
    return dict(**cols, open_time=ts, stress=stress, long_score=lng, short_score=sht, momentum=mom, context_ok=ctx,
                kind_at=kind_at, lens=lens, first_t=first)


def market_cases(seed: int = SEED + 5, n: int = 500):
    """Stand-in contexts for the two market methods: every value set holds
    the thresholds, their neighbours and NaN (momentum NaN: unavailable)."""
    g = np.random.default_rng(seed)
    pick = lambda xs: np.array(xs)[g.integers(0, len(xs), n)]   # noqa: E731
    return dict(context_ok=g.random(n) > 0.06,
                stress=np.where(g.random(n) < 0.5, pick((0.0, 0.2, 0.3499, 0.35, 0.3501, 0.6, np.nan)), 0.1),
                long_score=pick((0.2, 0.5, 0.5000001, 0.7, np.nan)), short_score=pick((0.1, 0.5, 0.6, np.nan)),
                momentum=pick((-2.0, -0.5000001, -0.5, -0.4999, 0.0, 0.4999, 0.5, 0.5000001, 3.0, np.nan, np.nan)))


def source_cases(seed: int = SEED + 6, n: int = 500):
    """last_spike stand-ins for source_spike_allows."""
    g = np.random.default_rng(seed)
    flag = lambda p: g.random(n) < p   # noqa: E731
    cor = np.array((-0.01, 0.0, 0.03, 0.0599, 0.06, 0.0600001, 0.2, np.nan))[g.integers(0, 8, n)]
    return dict(label=flag(0.8), price_break_flag=flag(0.4), cumulative_price_break_flag=flag(0.3),
                accel_spike_flag=flag(0.2), close_open_ratio=cor, upward=flag(0.7))


def digest(panel: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for f in sorted(panel):
        h.update(f.encode())
        h.update(np.ascontiguousarray(panel[f]).tobytes())
    return h.hexdigest()
