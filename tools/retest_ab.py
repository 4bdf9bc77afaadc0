"""Timing of the gradual-gainer retest replay (bq_retest.hip) beside three
launches of the same panel that read or walk it in comparable ways, at the
strategy rows' shape.

    python tools/retest_ab.py [--symbols 12500] [--candles 2000] [--rounds 7] [--out profiles/retest_ab.txt]

  (i)   engine.retest_replay (one launch): every output column, and the event
        column only
  (ii)  engine.cooldown (bq_cooldown): the same one-wave-per-row, 64-candles-
        per-step walk over one byte column (2 B out per candle)
  (iii) signals.impulse_rider_features, status only (bq_impulse_rider): a
        thread-per-candle stencil over the same OHLC + one more column
  (iv)  signals.gradual_gainer_leadership (bq_leadership): the launch that
        produces the replay's leader column

Nothing else computes the replay, so there is no A/B: the three neighbours
say what a pass over this panel costs. The variants alternate within each
round; HIP events time each call after warm-up. The bandwidth fraction counts
the replay's algorithmic bytes (5 fp64 columns + the open time + two flag
bytes in = 50 B, event + detail + level out = 10 B per candle; 51 B event
only) against 8 TB/s.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, signals   # noqa: E402

NAN = float("nan")
PEAK = 8.0e12


def make_panel(S: int, T: int, seed: int = 1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *sh: torch.rand(*sh, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    r = torch.randn(S, T, device="cuda", dtype=torch.float64, generator=g) * 0.005
    t = torch.arange(T, device="cuda")
    burst = ((t[None, :] + torch.randint(0, 60, (S, 1), device="cuda", generator=g)) % 60) < 8
    r = torch.where(burst, r + 0.008, r)
    c = 10.0 ** (rnd(S, 1) * 5 - 2) * torch.exp(torch.cumsum(r, dim=1))
    o = torch.cat([c[:, :1], c[:, :-1]], dim=1)
    h = torch.maximum(o, c) * (1 + 0.004 * rnd(S, T))
    l = torch.minimum(o, c) * (1 - 0.004 * rnd(S, T))
    atr = c * (0.01 + 0.06 * rnd(S, T))
    grid = 1_760_400_000_000 + 900_000 * torch.arange(T, device="cuda", dtype=torch.int64)
    ts = grid.expand(S, T).contiguous()
    bc = 60000.0 * torch.exp(torch.cumsum(torch.randn(T, device="cuda", dtype=torch.float64, generator=g) * 0.001,
                                          dim=0))
    risk = rnd(S, T) < 0.7
    return o, h, l, c, atr, ts, grid.contiguous(), bc.contiguous(), risk


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, T = a.symbols, a.candles
    o, h, l, c, atr, ts, bts, bc, risk = make_panel(S, T)
    lead = signals.gradual_gainer_leadership(ts, c, bts, bc)
    leader = lead["leader"]
    ema20 = signals.ema(c, 20)
    del lead

    event, detail, level = engine.retest_replay(o, h, l, c, ema20, ts, leader, risk)
    counts = torch.bincount(event.flatten().to(torch.int64), minlength=6)[:6].tolist()
    expired = int(((detail & signals.RT_D_EXPIRED) != 0).sum())
    only, _, _ = engine.retest_replay(o, h, l, c, ema20, ts, leader, risk, detail=False, level=False)
    assert torch.equal(only, event), "event-only launch differs"
    del event, detail, level, only

    variants = {
        "retest replay, every column": lambda: engine.retest_replay(o, h, l, c, ema20, ts, leader, risk),
        "retest replay, event only": lambda: engine.retest_replay(o, h, l, c, ema20, ts, leader, risk, detail=False,
                                                                  level=False),
        "cooldown (bq_cooldown)": lambda: engine.cooldown(leader, 3),
        "impulse rider, status only": lambda: signals.impulse_rider_features(o, h, l, c, atr, ts, bts, bc, columns=(),
                                                                             check_bench=False),
        "leadership (bq_leadership)": lambda: signals.gradual_gainer_leadership(ts, c, bts, bc),
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
    nbytes = {"retest replay, every column": 60, "retest replay, event only": 51}
    lines = [f"retest_ab: {S} x {T} on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating; events idle / watch_set / watching / risk_blocked / candidate / short = {counts}, "
             f"{expired} expiries",
             f"{'variant':32s} {'median ms':>10s} {'min':>8s} {'max':>8s}  fraction of 8 TB/s (algorithmic bytes)"]
    for name, ts_ in times.items():
        med = statistics.median(ts_)
        frac = f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} at {nbytes[name]} B/candle" if name in nbytes else ""
        lines.append(f"{name:32s} {med:10.3f} {min(ts_):8.3f} {max(ts_):8.3f}  {frac}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
