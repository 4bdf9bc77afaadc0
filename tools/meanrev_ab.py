"""Timing of the mean-reversion-fade replay (bq_meanrev.hip), in one process:
the kernel at the strategy rows' shape beside the staged feature pipeline that
exists without it.

    timeout -k 10 600 python tools/meanrev_ab.py [--symbols 12500] [--candles 2000] [--rounds 9] \\
        [--out profiles/meanrev_ab.txt]

  (i)   signals.mean_reversion_fade_entry, every column: open, high, low,
        close, volume, atr, bb_upper and open_time [S, T] in, the snapshot
        entry [S, T] (18 B), the features formed in the pass; status and the
        seven value columns out
  (ii)  the same inputs, status only
  (iii) the same with mean_reversion_features' five columns given (five more
        columns in), every column out
  (iv)  signals.mean_reversion_features alone: one rolling_many launch plus a
        fused element-wise program; close, volume, atr, high, low, open in
        (close again for the second launch), six columns out. It decides
        nothing, so it is a lower bound of any staged composition.

The variants alternate within each round; HIP events time each call after
warm-up. The bandwidth fraction counts each variant's algorithmic bytes per
candle against 8 TB/s: (i) 8 x 8 + 18 in, 1 + 7 x 8 out = 139; (ii) 82 + 1 =
83; (iii) 13 x 8 + 18 + 57 = 179; (iv) 7 x 8 in + 6 x 8 out = 104. The
context rows ([5, T]) stay in L2 and are not counted.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, signals                # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
STEP_MS = 900_000


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


def table(times, note):
    lines = [f"{'variant':44s} {'median ms':>10s} {'min':>8s} {'max':>8s}"]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{name:44s} {med:10.4f} {min(ts):8.4f} {max(ts):8.4f}  {note(name, med)}")
    return lines


def kernel_part(S, T, rounds, warmup):
    p = device_panel(S, T, seed=3)
    o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
    atr = engine.enrich(o, h, l, c, v, columns=("ATR",))["ATR"]
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    bb = c * (0.995 + 0.01 * rnd(S, T))
    ot = (1_700_000_000_000 + STEP_MS * torch.arange(T, device="cuda", dtype=torch.int64)).expand(S, T).contiguous()
    ctx = torch.stack([0.3 * rnd(T), 0.2 + 0.2 * rnd(T), 0.3 + 0.2 * rnd(T), rnd(T) - 0.7, 0.01 * (rnd(T) - 0.5)])
    ctx_ok = rnd(T) > 0.08
    kind = (5 * rnd(S, T)).to(torch.uint8)
    sym = {"ok": kind != 0, "atr_pct": 0.004 + 0.03 * rnd(S, T), "trend_score": 0.01 * (rnd(S, T) - 0.6),
           "micro_regime": torch.where(kind == 4, 0, 2).to(torch.uint8),
           "micro_transition": torch.where(kind == 3, 1, 255).to(torch.uint8)}
    entry = lambda **kw: signals.mean_reversion_fade_entry(o, h, l, c, v, atr, bb, ot, ctx, ctx_ok, sym=sym, **kw)   # noqa: E731
    staged = signals.mean_reversion_features(o, h, l, c, v, atr)
    own = entry(columns=())["status"]
    given = entry(features=staged, columns=())["status"]
    counts = torch.bincount(own.flatten().to(torch.int64), minlength=len(signals.MR_REASONS))
    differ = int((own != given).sum())
    summary = (f"status 0..16 = {counts.tolist()}; cells where the in-pass features decide otherwise than the staged "
               f"ones: {differ}")
    del own, given

    variants = {
        "(i) replay, every column": lambda: entry(),
        "(ii) replay, status only": lambda: entry(columns=()),
        "(iii) replay, features given": lambda: entry(features=staged),
        "(iv) staged mean_reversion_features alone": lambda: signals.mean_reversion_features(o, h, l, c, v, atr),
    }
    nbytes = dict(zip(variants, (139, 83, 179, 104)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    times = timed(variants, rounds, warmup)
    a, b = sorted(times["(i) replay, every column"]), sorted(times["(iv) staged mean_reversion_features alone"])
    q = lambda x: (x[len(x) // 4], x[(3 * len(x)) // 4])   # noqa: E731  (quartiles of the sorted samples)
    verdict = (f"(i) against (iv): medians {statistics.median(a):.4f} / {statistics.median(b):.4f} ms, difference "
               f"{statistics.median(b) - statistics.median(a):.4f} ms; run-to-run spread max - min "
               f"{a[-1] - a[0]:.4f} / {b[-1] - b[0]:.4f} ms, quartiles {q(a)[0]:.4f}-{q(a)[1]:.4f} / "
               f"{q(b)[0]:.4f}-{q(b)[1]:.4f} ms; (i) max {a[-1]:.4f} {'<' if a[-1] < b[0] else '>='} (iv) min "
               f"{b[0]:.4f}")
    return [f"kernel: {S} x {T}; {summary}"] + table(times, note) + [verdict, "PMC counters: not measured"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"meanrev_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating"]
    lines += kernel_part(a.symbols, a.candles, a.rounds, a.warmup)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
