#!/usr/bin/env python3
"""Pin the output bits of the five wave-per-row replay entry points whose
device code moved when their scaffolding went to csrc/bq_replay.h: the cases
and their digests.

`make isa-digest` shows which kernel files compile to the parent commit's
assembly (profiles/replay_isa.txt); bq_retest, bq_spikefade, bq_pricetracker,
bq_meanrev and bq_rangefade do not, so their entry points are compared here,
bit for bit, with the library of the parent commit.
tests/test_replay_parent_bits_gpu.py runs the cases; this file holds what the
test and the fixture writer share and, run as a script, writes the fixture:

  BQ_LIB_PATH=<library built from the parent commit> \\
      python tools/replay_parent_bits.py --commit <parent id> --out tests/golden/replay_parent_bits.json

The fixture is written from the parent's library only: BQ_LIB_PATH must be set
and must not name this tree's own library. It holds one SHA-256 per output
array and per state array after the call, so a NaN's payload and the sign of
a zero count.

Every case has S = 6 rows (two workgroups of four waves, the second half
empty) built on the host by the generators of tests/*_cases.py:

  row 0  the whole row                       row 3  lens = T - 3
  row 1  first_t = 5 (mid-step)              row 4  first_t = 7
  row 2  first_t = 1, from_t = 129: the      row 5  from_t = T >= lens: no
         steps at 0 and 64 only warm up             replayed candle

T = 1 / 63 / 64 / 65 / 130 / 200 with the entry's heaviest configuration
(features formed in the pass, per-candle context and snapshot, state given,
every column). Price tracker and mean reversion at T = 130 / 200 hold, inside
the frames: a NaN close at candle 70 of row 1 (the second step of its frame:
the row turns serial with a seeded carry), a NaN close at row 4's first_t
itself, a +inf close (row 0, candle 90) and 20 equal closes (row 3, from 40).
At T = 200 the variants follow: price tracker tail_rows 1, cooldown_ms 0 and
3 candles, h / l / v not given, trend_score given; mean reversion's windows
at _lib.MR_MAX_WINDOW, range fade's at their _lib maxima; features given; the
context as one column with one snapshot entry per row; no snapshot, no state
and a one-column subset; every input a slice of a wider tensor (row pitch
T + 1). Retest and spike fade: state, risk / market masks and optional
outputs given and not, the market masks as one shared [T] row, and the wider
row pitch.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 20261020
S = 6
SHAPES = (1, 63, 64, 65, 130, 200)
TV = 200   # the variants' T
NAN_SECOND_STEP, INF_AT, FLAT = (1, 70), (0, 90), (3, 40, 20)   # (row, candle[, length])
VARIANTS = {
    "retest": ("bare", "pitch"),
    "spike_fade": ("shared", "bare", "pitch"),
    "price_tracker": ("tail1", "cd0", "cd3", "nohlv", "trend", "ctx1", "bare", "pitch"),
    "mean_reversion": ("wmax", "feat", "ctx1", "bare", "pitch"),
    "range_fade": ("wmax", "feat", "ctx1", "bare", "pitch"),
}
CASES = [(e, T, "base") for e in VARIANTS for T in SHAPES] + [(e, TV, v) for e, vs in VARIANTS.items() for v in vs]


def case_id(case) -> str:
    return "{}/{}/{}".format(*case)


def rows(T: int) -> dict[str, np.ndarray]:
    """lens / first_t / from_t of the six rows (see the module's docstring)"""
    return dict(lens=np.array([T, T, T, max(T - 3, 0), T, T], np.int64),
                first_t=np.array([0, 5, 1, 0, 7, 0], np.int64),
                from_t=np.array([0, 0, 129, 0, 0, T], np.int64))


def _plant_closes(close: np.ndarray, T: int) -> None:
    """the serial switch's cases, inside the frames of rows() (T >= 130)"""
    if T < 130:
        return
    r = rows(T)
    close[NAN_SECOND_STEP] = np.nan
    close[4, r["first_t"][4]] = np.nan
    close[INF_AT] = np.inf
    s, a, n = FLAT
    close[s, a:a + n] = close[s, a]


def inputs(entry: str, T: int) -> dict:
    """the entry's host inputs at T candles, from the generators of tests/*_cases.py"""
    seed = SEED + 7 * T
    r = rows(T)
    if entry == "retest":
        import retest_cases as rc

        assert rc.EDGE_S == S
        p = rc.edge_panel(T, seed)
    elif entry == "spike_fade":
        import spikefade_cases as sc

        p = sc.edge_panel(S, T, seed)
    elif entry == "price_tracker":
        import pricetracker_cases as pc

        p = pc.seeded_panel(S, T, seed)
        _plant_closes(p["close"], T)
        p["trend_score"] = np.random.default_rng(seed + 1).normal(0.03, 0.02, (S, T))
    elif entry == "mean_reversion":
        import meanrev_cases as mc

        p = mc.seeded_panel(S, T, seed, first_t=r["first_t"])
        _plant_closes(p["close"], T)
        p["features"] = mc.random_features(p, seed + 1)
    elif entry == "range_fade":
        import rangefade_cases as fc

        nans = (("close", 1, 70), ("high", 4, 7)) if T >= 130 else ()
        p = fc.seeded_panel(S, T, seed, first_t=r["first_t"], nans=nans)
        g = np.random.default_rng(seed + 1)
        p["features"] = dict(adx=g.uniform(5.0, 45.0, (S, T)), zscore=g.normal(0.0, 2.0, (S, T)))
    else:
        raise ValueError(entry)
    p.update(r)
    return p


def _dev(x, dev, pad: int = 0):
    """a host array on the device; pad > 0: the first T columns of a [S, T + pad] buffer"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if pad and t.dim() == 2 and t.shape[0] == S:
        buf = torch.zeros((t.shape[0], t.shape[1] + pad), dtype=t.dtype, device=dev)
        buf[:, :t.shape[1]] = t
        t = buf[:, :t.shape[1]]
        assert t.stride(0) == x.shape[1] + pad
    return t


def _state(entry: str, p: dict, dev):
    """a carried-in state that holds an entry on the odd rows"""
    import torch

    odd = (np.arange(S) % 2).astype(np.uint8)
    T = p["close"].shape[1]
    at = min(2, T - 1)
    if entry == "retest":
        st = (odd, np.where(odd, p["open_time"][:, at], 0), np.where(odd, p["high"][:, at], np.nan))
    elif entry == "spike_fade":
        st = (odd, np.where(odd, p["open_time"][:, at], 0), np.where(odd, p["high"][:, at], np.nan),
              np.where(odd, p["close"][:, at], np.nan))
    elif entry == "price_tracker":
        st = (odd, np.where(odd, p["close_time"][:, at], 0))
    else:
        st = (odd, np.where(odd, p["open_time"][:, at], 0))
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in st)


def run_case(case, dev) -> dict[str, np.ndarray]:
    """the case's output and state arrays, on the host"""
    import torch

    from binquant_amd import _lib, engine

    entry, T, var = case
    p = inputs(entry, T)
    pad = 1 if var == "pitch" else 0
    bare = var == "bare"
    d = lambda k: _dev(p[k], dev, pad)   # noqa: E731
    rws = dict(lens=_dev(p["lens"], dev), first_t=_dev(p["first_t"], dev), from_t=_dev(p["from_t"], dev))
    state = None if bare or entry == "range_fade" else _state(entry, p, dev)
    ctx1 = var == "ctx1"
    out = {}
    if entry == "retest":
        ev, det, lvl = engine.retest_replay(
            d("open"), d("high"), d("low"), d("close"), d("ema"), d("open_time"), d("leader"),
            None if bare else d("risk_ok"), state=state, detail=not bare, level=True,
            min_history=12, watch_ms=20 * 900_000, breakout_lookback=8, **rws)
        out = dict(event=ev, detail=det, level=lvl)
    elif entry == "spike_fade":
        sm, fm = (None, None) if bare else (d("src_market"), d("fail_market"))
        if var == "shared":
            sm, fm = _dev(p["src_market"][0], dev), _dev(p["fail_market"][0], dev)
        ev, det, brs = engine.spike_fade_replay(d("open"), d("high"), d("close"), d("open_time"), d("source_ok"), sm,
                                                fm, state=state, detail=not bare, bars=True, **rws)
        out = dict(event=ev, detail=det, bars=brs)
    elif entry == "price_tracker":
        par = {"tail1": dict(tail_rows=1), "cd0": dict(cooldown_ms=0), "cd3": dict(cooldown_ms=3 * 300_000)}
        par = par.get(var, {})
        hlv = {} if var == "nohlv" else dict(h=d("high"), l=d("low"), v=d("volume"))
        ctx, ok, rs = p["ctx"], p["ctx_ok"], p["symbol_rs"]
        if ctx1:
            ctx, ok, rs = ctx[:, :1], ok[:1], rs[:, 0]
        st, det, vals = engine.price_tracker_replay(
            d("close"), d("rsi"), d("macd"), d("mfi"), d("close_time"), _dev(rs, dev, pad), _dev(ctx, dev),
            _dev(ok, dev),
            trend_score=d("trend_score") if var == "trend" else None, state=state, detail=not bare,
            columns=_lib.PT_VALUES[-1:] if bare else _lib.PT_VALUES, **hlv, **par, **rws)
        out = dict(status=st, detail=det, **vals)
    else:
        mr = entry == "mean_reversion"
        keys = [k for k, _ in (engine._MR_SYM if mr else engine._RF_SYM)]
        names = dict(ok="ok", atr_pct="atr_pct", trend_score="trend_score", regime="micro_regime",
                     transition="micro_transition", micro_regime="micro_regime", micro_transition="micro_transition",
                     bb_width="bb_width")
        sym = None
        if not bare:
            sym = tuple(_dev(p["sym"][names[k]][:, 0] if ctx1 else p["sym"][names[k]], dev) for k in keys)
        ctx, ok = (p["ctx"][:, :1], p["ctx_ok"][:1]) if ctx1 else (p["ctx"], p["ctx_ok"])
        values = _lib.MR_VALUES if mr else _lib.RF_VALUES
        nfeat = _lib.MR_NFEATURES if mr else _lib.RF_NFEATURES
        feats = tuple(_dev(p["features"][k], dev, pad) for k in values[:nfeat]) if var == "feat" else None
        cols = values[-1:] if bare else values
        if mr:
            par = dict(max_trend_score=0.06)
            if var == "wmax":
                par.update(volume_ma_window=_lib.MR_MAX_WINDOW, atr_ma_window=_lib.MR_MAX_WINDOW)
            st, vals = engine.mean_reversion_replay(
                d("open"), d("high"), d("low"), d("close"), d("volume"), d("atr"), d("bb_upper"), d("open_time"),
                _dev(ctx, dev), _dev(ok, dev), sym=sym, features=feats, state=state, columns=cols, **par, **rws)
        else:
            par = {}
            if var == "wmax":
                par = dict(adx_window=_lib.RF_MAX_ADX_WINDOW, zscore_window=_lib.RF_MAX_ZSCORE_WINDOW)
            st, vals = engine.range_fade_replay(
                d("open"), d("high"), d("low"), d("close"), d("volume"), d("rsi"), d("bb_upper"), d("bb_mid"),
                d("bb_lower"), _dev(ctx, dev), _dev(ok, dev), sym=sym, features=feats, columns=cols, **par, **rws)
        out = dict(status=st, **vals)
    torch.cuda.synchronize()
    out = {k: v for k, v in out.items() if v is not None}
    out.update({f"state{i}": x for i, x in enumerate(state or ())})
    return {k: v.cpu().numpy() for k, v in out.items()}


def digests(out: dict[str, np.ndarray]) -> dict[str, str]:
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="id of the commit the library in BQ_LIB_PATH was built from")
    ap.add_argument("--out", required=True, help="fixture to write (tests/golden/replay_parent_bits.json)")
    args = ap.parse_args()
    lib = os.environ.get("BQ_LIB_PATH")
    own = os.path.join(ROOT, "binquant_amd", "lib", "libbinquant_amd.so")
    if not lib or os.path.realpath(lib) == os.path.realpath(own):
        print("BQ_LIB_PATH must name a library built from the parent commit, not this tree's own: the fixture "
              "is never written from the code under test", file=sys.stderr)
        return 2
    if len(args.commit) != 40:
        print("--commit: the full 40-character id", file=sys.stderr)
        return 2
    import torch

    from binquant_amd import _lib

    dev = torch.device("cuda:0")
    doc = {"parent_commit": args.commit, "seed": SEED, "library": _lib.load().bq_version().decode(),
           "digests": {case_id(c): digests(run_case(c, dev)) for c in CASES}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {sum(len(d) for d in doc['digests'].values())} digests from {_lib.LIB_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
