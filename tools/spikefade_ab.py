"""Timing of the failed-spike-fade replay (bq_spikefade.hip) beside two
unchanged launches with the same one-wave-per-row, 64-candles-per-step walk,
in one process, at the strategy rows' shape.

    timeout -k 10 300 python tools/spikefade_ab.py [--symbols 12500] [--candles 2000] [--rounds 3] \\
        [--out profiles/spikefade_ab.txt]

  (i)   engine.spike_fade_replay (one launch): every output column, and the
        event column only
  (ii)  engine.retest_replay (bq_retest_replay): the sibling walk, 60 B per
        candle — the yardstick: the new kernel moves fewer bytes and should
        not be slower in the same run
  (iii) engine.cooldown (bq_cooldown): the same walk over one byte column

Nothing else computes the replay, so there is no A/B of its result: the two
neighbours say what a pass of this shape costs. The variants alternate within
each round; HIP events time each call after warm-up. The bandwidth fraction
counts the replay's algorithmic bytes (3 fp64 columns + the open time + the
source byte in = 33 B, the two market bytes of one shared [T] row not
counted, event + detail + bars out = 3 B per candle; 34 B event only)
against 8 TB/s.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, signals   # noqa: E402
from retest_ab import make_panel           # noqa: E402  (the same panel as the retest timing)

PEAK = 8.0e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, T = a.symbols, a.candles
    o, h, l, c, atr, ts, bts, bc, risk = make_panel(S, T)
    leader = signals.gradual_gainer_leadership(ts, c, bts, bc)["leader"]
    ema20 = signals.ema(c, 20)
    g = torch.Generator(device="cuda").manual_seed(2)
    # a source about every 40 candles (the bursts of the panel carry green runs), the market gates as [T] rows
    source = (torch.rand(S, T, device="cuda", generator=g) < 0.025) & (c > o)
    src_m = torch.rand(T, device="cuda", generator=g) < 0.7
    fail_m = torch.rand(T, device="cuda", generator=g) < 0.4

    event, detail, bars = engine.spike_fade_replay(o, h, c, ts, source, src_m, fail_m)
    counts = torch.bincount(event.flatten().to(torch.int64), minlength=6)[:6].tolist()
    cleared = {k: int(((event == signals.FS_CLEARED) & ((detail & b) != 0)).sum())
               for k, b in (("window", signals.FS_D_WINDOW_EXPIRED), ("extension", signals.FS_D_EXTENSION))}
    only, _, _ = engine.spike_fade_replay(o, h, c, ts, source, src_m, fail_m, detail=False, bars=False)
    assert torch.equal(only, event), "event-only launch differs"
    del event, detail, bars, only

    variants = {
        "spike fade replay, every column": lambda: engine.spike_fade_replay(o, h, c, ts, source, src_m, fail_m),
        "spike fade replay, event only": lambda: engine.spike_fade_replay(o, h, c, ts, source, src_m, fail_m,
                                                                          detail=False, bars=False),
        "retest replay, every column": lambda: engine.retest_replay(o, h, l, c, ema20, ts, leader, risk),
        "cooldown (bq_cooldown)": lambda: engine.cooldown(leader, 3),
    }
    times = {k: [] for k in variants}
    for rnd in range(a.warmup + a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            e1.synchronize()
            del res
            if rnd >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    nbytes = {"spike fade replay, every column": 36, "spike fade replay, event only": 34,
              "retest replay, every column": 60}
    lines = [f"spikefade_ab: {S} x {T} on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating; events idle / source_set / waiting / candidate / cleared / same_candle = {counts}, "
             f"cleared by {cleared}",
             f"{'variant':34s} {'median ms':>10s} {'min':>8s} {'max':>8s}  fraction of 8 TB/s (algorithmic bytes)"]
    for name, ts_ in times.items():
        med = statistics.median(ts_)
        frac = f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} at {nbytes[name]} B/candle" if name in nbytes else ""
        lines.append(f"{name:34s} {med:10.3f} {min(ts_):8.3f} {max(ts_):8.3f}  {frac}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
