"""Cost of the fresh panel context build on the GPU.

Times, with HIP events on the launch stream after a warm-up and with the
variants interleaved inside every repeat:

  compact        bq_panel_compact        (panel_compact_kernel)
  features       bq_market_features on the compacted panel
  breadth_fresh  bq_breadth_partial_fresh (breadth_kernel<FRESH>, bq_breadth.hip)
  breadth_dense  bq_breadth_partial on the same all-present features — the
                 kernel the fresh one is measured against

on an all-present panel and on one with 10 % of the candles absent, at
12 500 x 2 000 and at the 12 500 x 10 000 shard. Bytes per second are the
bytes the algorithm needs over the kernel's time: compaction 24 B read +
28 B written per candle; gather 4 B of rank per element + 56 B per fresh
candle; dense breadth 56 B per element.

    python tools/fresh_context_cost.py [--out FILE] [--repeats 7] [--shapes 12500x2000,12500x10000]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from binquant_amd import engine  # noqa: E402
from binquant_amd._lib import FEATURE_COLUMNS, PARTIAL_COLUMNS  # noqa: E402
from binquant_amd.synth import device_panel  # noqa: E402

MAX_BARS = 400


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(S: int, T: int, repeats: int, emit) -> None:
    p = device_panel(S, T, seed=77)
    h, l, c = p["high"], p["low"], p["close"]
    del p
    absent = torch.rand((S, T), device=c.device, generator=torch.Generator(c.device).manual_seed(5)) < 0.10
    nan = torch.full_like(c, float("nan"))
    hs, ls, cs = (torch.where(absent, nan, x) for x in (h, l, c))
    del nan
    n_fresh = {"all": S * T, "sparse": int((~absent).sum().item())}
    del absent
    panels = {"all": (h, l, c), "sparse": (hs, ls, cs)}
    comp = {k: engine.compact_panel(*v) for k, v in panels.items()}
    feats = {k: engine.market_features(comp[k].high, comp[k].low, comp[k].close, max_bars=MAX_BARS) for k in panels}
    out = torch.empty((T, len(PARTIAL_COLUMNS)), dtype=torch.float64, device=c.device)
    fbuf = {n: torch.empty_like(c) for n in FEATURE_COLUMNS}
    # what is timed launches only: outputs preallocated, validate=False (no sync)
    cbuf = None

    def run_compact(k):
        nonlocal cbuf
        cbuf = engine.compact_panel(*panels[k], validate=False)

    variants = {}
    for k in panels:
        variants[f"compact/{k}"] = (lambda k=k: run_compact(k), S * T * 52)
        variants[f"features/{k}"] = (lambda k=k: engine.market_features(comp[k].high, comp[k].low, comp[k].close,
                                                                         max_bars=MAX_BARS, out=fbuf), None)
        variants[f"breadth_fresh/{k}"] = (lambda k=k: engine.breadth_partial_fresh(comp[k], feats[k], out=out),
                                          S * T * 4 + n_fresh[k] * 56)
    variants["breadth_dense/all"] = (lambda: engine.breadth_partial(c, feats["all"], out=out), S * T * 56)
    for fn, _ in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (fn, _) in variants.items():
            times[k].append(timed(fn))
    emit(f"shape {S} x {T}, max_bars {MAX_BARS}, {repeats} interleaved repeats; "
         f"sparse panel: {100.0 * (1 - n_fresh['sparse'] / (S * T)):.1f} % of the candles absent")
    emit(f"  {'kernel/panel':24s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'TB/s':>7s}")
    med = {}
    for k, (_, nbytes) in variants.items():
        med[k] = statistics.median(times[k])
        rate = f"{nbytes / (med[k] * 1e-3) / 1e12:7.2f}" if nbytes else "      -"
        emit(f"  {k:24s} {med[k]:10.3f} {min(times[k]):9.3f} {max(times[k]):9.3f} {rate}")
    for k in panels:
        total = med[f"compact/{k}"] + med[f"features/{k}"] + med[f"breadth_fresh/{k}"]
        emit(f"  fresh build ({k}): compact + features + breadth_fresh = {total:.3f} ms")
    dense = med["features/all"] + med["breadth_dense/all"]
    emit(f"  dense unfused build: features + breadth_dense = {dense:.3f} ms")
    emit(f"  breadth_fresh / breadth_dense on the all-present panel: "
         f"{med['breadth_fresh/all'] / med['breadth_dense/all']:.2f}x")
    emit("")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="12500x2000,12500x10000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fresh_context_cost.py measures on the GPU; no HIP device is visible")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"fresh context build cost on {torch.cuda.get_device_name(0)} (HIP events, median of interleaved repeats)")
    for shape in a.shapes.split(","):
        S, T = (int(x) for x in shape.split("x"))
        measure(S, T, a.repeats, emit)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
