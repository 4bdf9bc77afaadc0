"""Cost of the per-symbol regime panel on the GPU.

Times, with HIP events on the launch stream after a warm-up and with the
variants interleaved inside every repeat, engine.symbol_regime_panel
(bq_symbol_regime_panel, symbol_regime_panel_kernel):

  dense/full      a dense build's columns, every context valid: each tile on
                  the in-order path
  dense/status    the same with the five columns range_fade_entry's sym reads
  fresh/full      a fresh build with 10 % of the candles absent (through rank)
  carried/full    the dense columns with 10 % of the contexts invalid and the
                  provider's carry: every tile gathers

next to breadth_kernel<FRESH> (bq_breadth_partial_fresh) on the same panels —
it reads the same seven columns through the same gather — and the host loop
the snapshot replaces: MarketContextBatch.symbol_features_at plus the label
encoding and the uploads, over 50 timestamps (host clock around a
synchronise; a per-timestamp cost, not extrapolated).

Bytes are the bytes the algorithm needs: 56 B read per candle, 4 B more with
rank, plus 1 B per requested flag / code column and 8 B per value column.

    python tools/regime_panel_cost.py [--out FILE] [--repeats 7] [--shapes 12500x2000,12500x10000]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from binquant_amd import _lib, engine  # noqa: E402
from binquant_amd.market_regime.batch import MarketContextBatch, seen_columns  # noqa: E402
from binquant_amd.market_regime.regime import ContextBatch  # noqa: E402
from binquant_amd.synth import device_panel  # noqa: E402

MAX_BARS = 400
PEAK = 8.0e12   # HBM3E bytes per second
STATUS = ("ok", "micro_regime", "micro_transition", "atr_pct", "bb_width")   # signals.RF_SYM_KEYS
HOST_STEPS = 50


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def out_bytes(columns) -> int:
    return sum(1 if k in _lib.REGIME_PANEL_U8 else 8 for k in columns)


def host_loop(batch: MarketContextBatch, close, steps: int) -> float:
    """Seconds per timestamp of the loop the snapshot replaces: one
    symbol_features_at, the codes of its labels, and the upload of the row."""
    reg = {r: i for i, r in enumerate(_lib.MICRO_REGIMES)}
    T = close.shape[1]
    picks = np.linspace(1, T - 1, steps).astype(int)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in picks:
        f = batch.symbol_features_at(int(i), close, 0.001, btc_index=0)
        has = ~np.isnan(f["return_pct"])
        row = dict(ok=has.astype(np.uint8),
                   micro_regime=np.array([reg[x] for x in f["micro_regime"]], dtype=np.uint8),
                   above_ema20=f["above_ema20"].astype(np.uint8), above_ema50=f["above_ema50"].astype(np.uint8),
                   rs_vs_btc=f["relative_strength_vs_btc"], micro_regime_strength=f["micro_regime_strength"],
                   trend_score=f["trend_score"], atr_pct=f["atr_pct"], bb_width=f["bb_width"])
        up = [torch.from_numpy(v).cuda() for v in row.values()]
    torch.cuda.synchronize()
    del up
    return (time.perf_counter() - t0) / steps


def measure(S: int, T: int, repeats: int, emit) -> None:
    p = device_panel(S, T, seed=77)
    h, l, c = p["high"], p["low"], p["close"]
    del p
    absent = torch.rand((S, T), device=c.device, generator=torch.Generator(c.device).manual_seed(5)) < 0.10
    nan = torch.full_like(c, float("nan"))
    comp_s = engine.compact_panel(*(torch.where(absent, nan, x) for x in (h, l, c)))
    del nan, absent
    comp_a = engine.compact_panel(h, l, c)
    feats = engine.market_features(h, l, c, max_bars=MAX_BARS)
    feats_s = engine.market_features(comp_s.high, comp_s.low, comp_s.close, max_bars=MAX_BARS)
    del h, l
    btc = feats["return_pct"][0].clone()
    valid = np.random.default_rng(6).random(T) >= 0.10
    at, prev = seen_columns(valid, np.arange(T), carry=True)
    at_d, prev_d = torch.from_numpy(at).cuda(), torch.from_numpy(prev).cuda()
    part = torch.empty((T, len(_lib.PARTIAL_COLUMNS)), dtype=torch.float64, device=c.device)
    full = _lib.REGIME_PANEL_COLUMNS
    n = S * T

    def panel(f, cl, cols, **kw):
        return lambda: engine.symbol_regime_panel(f, cl, btc_return=btc, btc_row=0, columns=cols, **kw)

    variants = {
        "regime dense/full": (panel(feats, c, full), n * (56 + out_bytes(full))),
        "regime dense/status": (panel(feats, c, STATUS), n * (56 + out_bytes(STATUS))),
        "regime fresh/full": (panel(feats_s, comp_s.close, full, rank=comp_s.rank), n * (60 + out_bytes(full))),
        "regime carried/full": (panel(feats, c, full, at=at_d, prev=prev_d), n * (56 + out_bytes(full))),
        "breadth_fresh/all": (lambda: engine.breadth_partial_fresh(comp_a, feats, out=part), n * 60),
        "breadth_fresh/sparse": (lambda: engine.breadth_partial_fresh(comp_s, feats_s, out=part), n * 60),
    }
    for fn, _ in variants.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (fn, _) in variants.items():
            times[k].append(timed(fn))
    emit(f"shape {S} x {T}, max_bars {MAX_BARS}, {repeats} interleaved repeats; fresh panel: 10 % of the candles "
         f"absent; carried: {100.0 * (1 - valid.mean()):.1f} % of the contexts invalid")
    emit(f"  {'kernel/case':24s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'GB moved':>9s} {'TB/s':>7s} "
         f"{'of 8 TB/s':>9s}")
    med = {}
    for k, (_, nbytes) in variants.items():
        med[k] = statistics.median(times[k])
        rate = nbytes / (med[k] * 1e-3)
        emit(f"  {k:24s} {med[k]:10.3f} {min(times[k]):9.3f} {max(times[k]):9.3f} {nbytes / 1e9:9.2f} {rate / 1e12:7.2f} "
             f"{100.0 * rate / PEAK:8.1f}%")
    scaled = med["breadth_fresh/all"] * (56 + out_bytes(full)) / 60
    emit(f"  regime dense/full against breadth_fresh/all scaled by the bytes moved ({scaled:.3f} ms): "
         f"{med['regime dense/full'] / scaled:.2f}x")
    cb = ContextBatch(timestamp=np.arange(T, dtype=np.int64), valid=np.ones(T, bool), fields={})
    per = host_loop(MarketContextBatch(contexts=cb, features=feats, partial=part), c, HOST_STEPS)
    emit(f"  host loop (symbol_features_at + codes + upload), {HOST_STEPS} timestamps timed: {per * 1e3:.3f} ms per "
         f"timestamp (host clock; {T} timestamps were not run)")
    emit("")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="12500x2000,12500x10000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regime_panel_cost.py measures on the GPU; no HIP device is visible")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"regime panel cost on {torch.cuda.get_device_name(0)} (HIP events, median of interleaved repeats)")
    for shape in a.shapes.split(","):
        S, T = (int(x) for x in shape.split("x"))
        measure(S, T, a.repeats, emit)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
