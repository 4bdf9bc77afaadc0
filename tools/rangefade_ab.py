"""Timing of the range-fade replay (bq_rangefade.hip), in one process: the
kernel at the strategy rows' shape beside the staged composition that exists
without it.

    timeout -k 10 600 python tools/rangefade_ab.py [--symbols 12500] [--candles 2000] [--rounds 3] \\
        [--out profiles/rangefade_ab.txt]

  (i)   signals.range_fade_entry, every column: open, high, low, close,
        volume, rsi and the three bands [S, T] in, the snapshot entry [S, T]
        (19 B), adx and zscore formed in the pass; status and the four value
        columns out
  (ii)  the same inputs, status only
  (iii) the same with signals.adx / signals.zscore's columns given (two more
        columns in), every column out
  (iv)  the staged lower bound: signals.adx + signals.zscore (one launch and
        one written column each) + the fused element-wise gate
        (binquant_amd.fused) over the same columns, whose only output is the
        pass bit. A fused program takes 16 operands and the gate reads 21, so
        it is two programs with a one-byte mask between them. The snapshot's
        two codes are handed to it as ready-made bool masks and the
        frame-length test as a [T] mask, it writes no reason and no value
        column: less than signal() needs, so a lower bound. The tool asserts
        that its pass bit equals status == 0 of (iii) on every cell.

The variants alternate within each round; HIP events time each call after the
warm-ups; median and min-max are reported. The bandwidth fraction counts each
variant's algorithmic bytes per candle against 8 TB/s: (i) 9 x 8 + 19 in, 1 +
4 x 8 out = 124; (ii) 91 + 1 = 92; (iii) 11 x 8 + 19 + 33 = 140; (iv) adx 3 x
8 + 8, zscore 8 + 8, the gate 6 x 8 + 19 in and 1 out, then 10 x 8 + 1 in and
1 out = 198. The context rows
([3, T]) stay in L2 and are not counted.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import _lib, engine, signals           # noqa: E402
from binquant_amd import fused as F                       # noqa: E402
from binquant_amd.synth import device_panel               # noqa: E402

PEAK = 8.0e12
P = engine.RANGE_FADE_DEFAULTS


def timed(variants, rounds, warmup):
    times = {k: [] for k in variants}
    for rnd in range(warmup + rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            e1.synchronize()
            del res
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return times


def staged_gate(o, h, l, c, v, rsi, bbu, bbm, bbl, adx, z, ctx, ctx_ok, enough, sym_ok, sym_range, sym_refused,
                sym_atr, sym_bbw):
    """The method's pass bit as fused element-wise programs (first_t = 0). A
    fused program takes 16 operands at most and the gate reads 21, so it is
    two programs: the frame, null and routing gates (16 operands) write a
    one-byte mask, the ADX cut and _resolve_entry (11 operands) read it."""
    O, H, L, C, V, R = (F.inp(x) for x in (o, h, l, c, v, rsi))
    nul = None
    for x in (O, H, L, C, R, V):
        for k in range(5):   # tail(5): the candle and the four before it
            n = F.isnan(F.shift(x, k) if k else x)
            nul = n if nul is None else nul | n
    trans, stress, regime = (F.inp(ctx[i]) for i in range(3))
    route = F.inp(ctx_ok) & (trans == 0.0) & ~(stress >= P["max_market_stress"]) & (regime == float(2)) \
        & F.inp(sym_ok) & F.inp(sym_range) & ~F.inp(sym_refused) & ~(F.inp(sym_atr) > P["max_symbol_atr_pct"]) \
        & ~(F.inp(sym_bbw) > P["max_symbol_bb_width"])
    routed = F.run({"routed": F.inp(enough) & ~nul & route})["routed"]
    U, M, D, A, Z = (F.inp(x) for x in (bbu, bbm, bbl, adx, z))
    rng = H - L
    live = ~(rng <= 0.0)
    pos = (C - L) / rng
    bull = live & (L <= D * (1.0 + P["band_touch_tolerance"])) & (C > O) \
        & ((F.where(C < O, C, O) - L) / rng >= P["min_rejection_wick_frac"]) & (pos >= P["long_close_position_min"])
    bear = live & (H >= U * (1.0 - P["band_touch_tolerance"])) & (C < O) \
        & ((H - F.where(C > O, C, O)) / rng >= P["min_rejection_wick_frac"]) & (pos <= P["short_close_position_max"])
    lng = (C <= M) & (R <= P["long_rsi_max"]) & (Z <= P["long_zscore_max"]) & bull
    sht = (C >= M) & (R >= P["short_rsi_min"]) & (Z >= P["short_zscore_min"]) & bear
    return F.run({"pass": F.inp(routed) & ~(A > P["adx_max"]) & (lng | sht)})["pass"]


def kernel_part(S, T, rounds, warmup):
    p = device_panel(S, T, seed=3)
    o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
    e = engine.enrich(o, h, l, c, v, columns=("rsi", "bb_upper", "bb_mid", "bb_lower"))
    rsi, bbu, bbm, bbl = (e[k] for k in ("rsi", "bb_upper", "bb_mid", "bb_lower"))
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    kind = (12 * rnd(T)).to(torch.int64)   # one context family per candle time: mostly RANGE and calm
    f64 = lambda x: x.to(torch.float64)   # noqa: E731
    ctx = torch.stack([f64(kind == 0), f64(torch.where(kind == 1, 0.6, 0.05)) + 0.2 * rnd(T),
                       f64(torch.where(kind == 2, float(_lib.MR_NONE), torch.where(kind == 3, 0.0, 2.0)))])
    ctx_ok = kind != 4
    sk = (12 * rnd(S, T)).to(torch.int64)
    sym = {"ok": sk != 0, "micro_regime": torch.where(sk == 1, 0, 2).to(torch.uint8),
           "micro_transition": torch.where(sk == 2, 1, 255).to(torch.uint8),
           "atr_pct": 0.004 + 0.03 * rnd(S, T) + 0.03 * f64(sk == 3),
           "bb_width": 0.01 + 0.06 * rnd(S, T) + 0.05 * f64(sk == 4)}
    entry = lambda **kw: signals.range_fade_entry(o, h, l, c, v, rsi, bbu, bbm, bbl, ctx, ctx_ok, sym=sym, **kw)   # noqa: E731

    adx, z = signals.adx(h, l, c), signals.zscore(c)
    enough = torch.arange(T, device="cuda") + 1 >= P["min_candles"]
    masks = (sym["ok"], sym["micro_regime"] == 2, sym["micro_transition"] <= 2)
    staged = lambda: staged_gate(o, h, l, c, v, rsi, bbu, bbm, bbl, signals.adx(h, l, c), signals.zscore(c), ctx,   # noqa: E731
                                 ctx_ok, enough, *masks, sym["atr_pct"], sym["bb_width"])
    own = entry(columns=())["status"]
    given = entry(features={"adx": adx, "zscore": z}, columns=())["status"]
    bit = staged()
    torch.cuda.synchronize()
    wrong = int((bit != (given == signals.RF_EMIT)).sum())
    assert wrong == 0, f"the staged gate's pass bit differs from status == 0 on {wrong} cells"
    counts = torch.bincount(own.flatten().to(torch.int64), minlength=len(signals.RF_REASONS))
    differ = int((own != given).sum())
    summary = (f"status 0..14 = {counts.tolist()}; cells where the in-pass features decide otherwise than the staged "
               f"ones: {differ}; the staged gate's pass bit equals status == 0 on all {S * T} cells")
    del own, given, bit

    variants = {
        "(i) replay, every column": lambda: entry(),
        "(ii) replay, status only": lambda: entry(columns=()),
        "(iii) replay, features given": lambda: entry(features={"adx": adx, "zscore": z}),
        "(iv) staged adx + zscore + fused gate": staged,
    }
    nbytes = dict(zip(variants, (124, 92, 140, 198)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    times = timed(variants, rounds, warmup)
    lines = [f"{'variant':44s} {'median ms':>10s} {'min':>8s} {'max':>8s}"]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{name:44s} {med:10.4f} {min(ts):8.4f} {max(ts):8.4f}  {note(name, med)}")
    a, b = times["(i) replay, every column"], times["(iv) staged adx + zscore + fused gate"]
    verdict = (f"(i) against (iv): medians {statistics.median(a):.4f} / {statistics.median(b):.4f} ms, difference "
               f"{statistics.median(b) - statistics.median(a):.4f} ms; (i) max {max(a):.4f} "
               f"{'<' if max(a) < min(b) else '>='} (iv) min {min(b):.4f}")
    return [f"kernel: {S} x {T}; {summary}"] + lines + [verdict, "PMC counters: not measured"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"rangefade_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating"]
    lines += kernel_part(a.symbols, a.candles, a.rounds, a.warmup)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
