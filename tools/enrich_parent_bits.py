#!/usr/bin/env python3
"""Pin bq_enrich's output bits: the edge-case panel and its digests.

tests/test_enrich_parent_bits_gpu.py compares the enrich kernels, bit for bit,
with the library of an earlier commit. This file holds what the test and the
fixture writer share — the panel (build_panel), the digest of an output
(digests) and the two ways of calling bq_enrich (run_hot, run_generic) — and,
run as a script, writes the fixture:

  BQ_LIB_PATH=<library built from the parent commit> \\
      python tools/enrich_parent_bits.py --commit <parent id> --out tests/golden/enrich_parent_bits.json

The fixture is written from the parent's library only (BQ_LIB_PATH must be
set), never from the tree under test. It holds a SHA-256 per (column, row,
256-candle block) of the output bytes, so a NaN's payload and the sign of a
zero count.

The panel: S = 6 rows at T = 2832 (two whole tiles plus the headline's
784-candle tail) and T = 1025. Row 0 is a plain numpy_panel walk. Rows 1..5
are walks with five kinds of segment written in, the cases the kernel's
selects decide:

  const   150 candles of constant close: same-value rule of ma_100 / bb_mid, sd 0, RSI NaN
  updown  40 strictly rising, then 40 strictly falling closes and typical prices: RSI / MFI 100 and 0
  novol   30 candles of zero volume: MFI NaN
  flat    20 identical OHLC bars: TR 0, a constant (o+h+l+c)/4 (same-value rule of ATR / TWAP)
  ulp     25 closes alternating between two adjacent doubles: variance at the rounding floor

and five placements of a segment's first candle (PLACES): inside the first
100 candles; inside one lane's 4 candles; on a lane boundary; across a wave
boundary (a multiple of 256); across the tile boundaries 1024 and 2048. Row
1 + r puts segment kind j at placement (r + j) % 5, so every (kind, placement)
pair occurs once and no two segments of a row overlap. A segment that does not
fit below T is clipped or dropped.
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

SEED = 20240611
S = 6
LENGTHS = (2832, 1025)
BLOCK = 256
KINDS = ("const", "updown", "novol", "flat", "ulp")
KIND_LEN = {"const": 150, "updown": 80, "novol": 30, "flat": 20, "ulp": 25}
PLACES = ("warmup", "in_lane", "lane_edge", "wave_edge", "tile_edge")


def starts(place: str, n: int) -> list[int]:
    """first candles of an n-candle segment at a placement (regions of
    different placements are disjoint for n <= 150)"""
    if place == "warmup":
        return [20]
    if place == "in_lane":      # the segment begins on a lane's second candle
        return [201]
    if place == "lane_edge":    # ... on a lane's first candle, not a wave's
        return [640]
    if place == "wave_edge":    # straddles candle 512 (tile 0) and 1536 (the steady loop's tile)
        return [512 - n // 2, 1536 - n // 2]
    if place == "tile_edge":    # straddles 1024 and 2048
        return [1024 - n // 2, 2048 - n // 2]
    raise ValueError(place)


def write_segment(p: dict[str, np.ndarray], row: int, kind: str, a: int, T: int) -> None:
    b = min(a + KIND_LEN[kind], T)
    if a < 1 or b - a < 2:
        return
    o, h, l, c, v = (p[f][row] for f in ("open", "high", "low", "close", "volume"))
    n = b - a
    if kind == "const":
        c[a:b] = c[a]
    elif kind == "updown":
        up = min(n, 40)
        step = c[a - 1] * 0.0007
        c[a:a + up] = c[a - 1] + step * np.arange(1, up + 1)
        if n > up:
            c[a + up:b] = c[a + up - 1] - step * np.arange(1, n - up + 1)
    elif kind == "novol":
        v[a:b] = 0.0
        return
    elif kind == "flat":
        c[a:b] = c[a]
    elif kind == "ulp":
        c[a:b] = np.where(np.arange(n) % 2 == 0, c[a], np.nextafter(c[a], np.inf))
    # the bars around the rewritten closes: open = previous close, and a
    # range that follows the close (typical price strictly monotone in updown)
    e = min(b + 1, T)
    o[a:e] = c[a - 1:e - 1]
    if kind == "flat":
        o[a:b] = h[a:b] = l[a:b] = c[a:b]
        v[a:b] = np.maximum(v[a:b], 1.0)
    else:
        h[a:b] = np.maximum(o[a:b], c[a:b]) * (1.0 + 0.001)
        l[a:b] = np.minimum(o[a:b], c[a:b]) * (1.0 - 0.001)
        if kind == "updown":
            h[a:b] = c[a:b] * (1.0 + 0.002)
            l[a:b] = c[a:b] * (1.0 - 0.002)
            v[a:b] = np.maximum(v[a:b], 1.0)
    if e > b:
        h[b] = max(h[b], o[b])
        l[b] = min(l[b], o[b])


def build_panel(T: int) -> dict[str, np.ndarray]:
    from binquant_amd.synth import numpy_panel

    p = numpy_panel(S, T, seed0=SEED + T)
    for r in range(S - 1):
        for j, kind in enumerate(KINDS):
            for a in starts(PLACES[(r + j) % len(PLACES)], KIND_LEN[kind]):
                write_segment(p, 1 + r, kind, a, T)
    assert all(np.isfinite(x).all() for x in p.values())
    return p


def digests(out: dict[str, np.ndarray]) -> dict[str, list[list[str]]]:
    """{column: [row][block] -> SHA-256 of the block's bytes}"""
    res = {}
    for col, x in out.items():
        x = np.ascontiguousarray(x, dtype=np.float64)
        res[col] = [[hashlib.sha256(row[t:t + BLOCK].tobytes()).hexdigest() for t in range(0, len(row), BLOCK)]
                    for row in x]
    return res


def device_inputs(panel, dev):
    import torch

    from binquant_amd._lib import INPUT_FIELDS

    return [torch.from_numpy(np.array(panel[f])).to(dev) for f in INPUT_FIELDS]


def run_hot(ins) -> dict[str, np.ndarray]:
    """all 14 columns in one call: enrich_kernel<.., HOT>"""
    import torch

    from binquant_amd import engine

    got = engine.enrich(*ins)
    torch.cuda.synchronize()
    return {c: x.cpu().numpy() for c, x in got.items()}


def run_generic(ins) -> dict[str, np.ndarray]:
    """all 14 columns from two calls that each omit one: the generic kernels"""
    import torch

    from binquant_amd import engine
    from binquant_amd._lib import ENRICH_COLUMNS

    a = engine.enrich(*ins, columns=ENRICH_COLUMNS[:-1])
    b = engine.enrich(*ins, columns=ENRICH_COLUMNS[1:])
    torch.cuda.synchronize()
    return {c: (a[c] if c in a else b[c]).cpu().numpy() for c in ENRICH_COLUMNS}


def mismatches(got: dict, want: dict) -> list[str]:
    """'column row r block b (candles lo..hi)' for every digest that differs"""
    bad = []
    for col, rows in want.items():
        for r, blocks in enumerate(rows):
            for b, d in enumerate(blocks):
                if got[col][r][b] != d:
                    bad.append(f"{col} row {r} block {b} (candles {b * BLOCK}..{(b + 1) * BLOCK - 1})")
    return bad


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="id of the commit the library in BQ_LIB_PATH was built from")
    ap.add_argument("--out", required=True, help="fixture to write (tests/golden/enrich_parent_bits.json)")
    args = ap.parse_args()
    if not os.environ.get("BQ_LIB_PATH"):
        print("BQ_LIB_PATH is not set: the fixture is written from the parent commit's library only", file=sys.stderr)
        return 2
    import torch

    from binquant_amd import _lib

    dev = torch.device("cuda:0")
    doc = {"parent_commit": args.commit, "seed": SEED, "block": BLOCK, "rows": S, "library": _lib.load().bq_version().decode(),
           "digests": {}}
    for T in LENGTHS:
        ins = device_inputs(build_panel(T), dev)
        hot, gen = digests(run_hot(ins)), digests(run_generic(ins))
        bad = mismatches(gen, hot)
        if bad:
            print(f"T={T}: the parent's generic kernels differ from its hot kernel: {bad[:8]}", file=sys.stderr)
            return 1
        doc["digests"][str(T)] = hot
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {sum(len(r) for t in doc['digests'].values() for c in t.values() for r in c)} digests "
          f"from {_lib.LIB_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
