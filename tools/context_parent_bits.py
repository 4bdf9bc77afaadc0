#!/usr/bin/env python3
"""Pin the output bits of the market-context entry points: the cases and
their digests.

tests/test_context_parent_bits_gpu.py compares bq_breadth_partial,
bq_breadth_partial_fresh, bq_market_features (both kernels),
bq_context_partials and bq_panel_compact, bit for bit, with the library of an
earlier commit. This file holds what the test and the fixture writer share —
the cases (CASES), their host panels (dense_panel, sparse_panel), the run of a
case (run_case) and the digest of its outputs — and, run as a script, writes
the fixture:

  BQ_LIB_PATH=<library built from the parent commit> \\
      python tools/context_parent_bits.py --commit <parent id> --out tests/golden/context_parent_bits.json

The fixture is written from the parent's library only (BQ_LIB_PATH must be
set), never from the tree under test. It holds one SHA-256 per output array,
so a NaN's payload and the sign of a zero count.

The cases, (S, T[, max_bars]):

  breadth        dense sums over market_features of an edges=True panel (its
                 candle 0 has no features: NaN returns). T = 1 / 3 / 256: the
                 workgroup-per-timestamp kernel, with fewer symbols than
                 threads and (S = 1500) more; T = 257 / 700: the lane-per-
                 timestamp kernel, with fewer symbols than waves (S = 5, last
                 block one lane wide) and more.
  breadth_fresh  the gathered sums on sparse_panel (both kernels), and one
                 panel with every candle present.
  features       the workgroup-per-symbol kernel (S < 4096): several tiles, a
                 short cap, and an odd row stride (the scalar load path).
  features_wave  the wave-per-symbol kernel (S = 4096, the router's threshold):
                 the D ring and the lagged chains.
  context        bq_context_partials with the last row's features; S is no
                 multiple of 4 (idle waves). max_bars 400 / 380: the ring with
                 the compile-time / run-time cap; 15: the lagged chains.
  compact        the compaction of sparse_panel: packed rows, tail, rank,
                 n_present, first_t.

sparse_panel follows tests/test_fresh_context_gpu.py: random gaps, a late
listing every 7th row, one never-present row, one delisted row (fewer than 7
rows: the last never present, the one before it late), plus one timestamp
where no symbol has a candle (T_EMPTY) and one where every symbol listed so
far has one (T_FULL).
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20241019
T_EMPTY, T_FULL = 40, 200
CASES = (
    [("breadth", S, T, 400) for S, T in ((5, 1), (70, 256), (1500, 3), (5, 257), (70, 700))]
    + [("breadth_fresh", S, T, 30) for S, T in ((70, 700), (70, 256), (5, 257))]
    + [("breadth_fresh_all", 70, 300, 30)]
    + [("features", 6, 2100, 512), ("features", 5, 60, 15), ("features_odd", 3, 1025, 400)]
    + [("features_wave", 4096, 300, 400), ("features_wave", 4096, 300, 15)]
    + [("context", 7, 255, 400), ("context", 9, 257, 400), ("context", 6, 700, 380), ("context", 5, 600, 15),
       ("context", 5, 60, 15)]
    + [("compact", 3, 257, 0)]
)


def case_id(case) -> str:
    kind, S, T, M = case
    return f"{kind}/{S}x{T}/{M}"


def dense_panel(S: int, T: int, edges: bool = True):
    """(high, low, close) of a numpy_panel"""
    from binquant_amd.synth import numpy_panel

    p = numpy_panel(S, T, seed0=SEED + 7 * S + T, edges=edges)
    return p["high"], p["low"], p["close"]


def sparse_panel(S: int, T: int):
    """(high, low, close, present): NaN where a candle is absent"""
    g = np.random.default_rng(SEED + 7 * S + T)
    h, l, c = dense_panel(S, T, edges=False)
    present = g.random((S, T)) < g.uniform(0.3, 1.0, S)[:, None]
    if S >= 7:
        late, never = range(0, S, 7), 5
        present[6, 300:] = False                        # delisted
    else:
        late, never = (S - 2,), S - 1
    for s in late:
        present[s, :g.integers(1, T - 1)] = False       # late listings
    present[never] = False
    listed = present[:, :T_FULL].any(axis=1)            # every symbol listed so far has a candle at T_FULL
    present[:, T_FULL] |= listed
    present[:, T_EMPTY] = False                         # nobody has a candle here
    nan = np.where(present, 1.0, np.nan)
    return h * nan, l * nan, c * nan, present


def host_inputs(case):
    kind, S, T, _ = case
    if kind in ("breadth_fresh", "compact"):
        return sparse_panel(S, T)[:3]
    return dense_panel(S, T, edges=kind != "breadth_fresh_all")


def run_case(case, dev) -> dict[str, np.ndarray]:
    """the case's output arrays, on the host"""
    import torch

    from binquant_amd import engine
    from binquant_amd._lib import FEATURE_COLUMNS

    kind, S, T, M = case
    hlc = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host_inputs(case)]
    if kind == "features_odd":   # an odd row stride: the scalar load path
        hlc = [torch.cat([x, x[:, :2]], dim=1)[:, :T] for x in hlc]
        assert hlc[0].stride(0) % 2 == 1
    out = {}
    if kind == "breadth":
        feats = engine.market_features(*hlc, max_bars=M)
        out["partial"] = engine.breadth_partial(hlc[2], feats)
    elif kind in ("breadth_fresh", "breadth_fresh_all"):
        comp = engine.compact_panel(*hlc)
        feats = engine.market_features(comp.high, comp.low, comp.close, max_bars=M)
        out["partial"] = engine.breadth_partial_fresh(comp, feats)
    elif kind in ("features", "features_odd", "features_wave"):
        out = dict(engine.market_features(*hlc, max_bars=M))
        assert tuple(out) == tuple(FEATURE_COLUMNS)
    elif kind == "context":
        part, last = engine.context_partials(*hlc, max_bars=M, last=True)
        out = {"partial": part, **{f"last_{k}": v for k, v in last.items()}}
    elif kind == "compact":
        comp = engine.compact_panel(*hlc)
        n = comp.n_present.cpu().numpy()
        for name, x in (("high", comp.high), ("low", comp.low), ("close", comp.close)):
            x = x.cpu().numpy()
            out[f"packed_{name}"] = np.concatenate([x[s, :n[s]] for s in range(S)])
            out[f"tail_{name}"] = np.concatenate([x[s, n[s]:] for s in range(S)])
        out.update(rank=comp.rank, n_present=comp.n_present, first_t=comp.first_t)
    else:
        raise ValueError(kind)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def digests(out: dict[str, np.ndarray]) -> dict[str, str]:
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="id of the commit the library in BQ_LIB_PATH was built from")
    ap.add_argument("--out", required=True, help="fixture to write (tests/golden/context_parent_bits.json)")
    args = ap.parse_args()
    if not os.environ.get("BQ_LIB_PATH"):
        print("BQ_LIB_PATH is not set: the fixture is written from the parent commit's library only", file=sys.stderr)
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
