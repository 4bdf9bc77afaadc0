"""Timing of the BB-extreme replay (bq_bbextreme.hip), in one process: the
kernel at the strategy rows' shape beside the staged composition that exists
without it and the same-mapping buy-the-dip replay.

    timeout -k 10 600 python tools/bbextreme_ab.py [--symbols 12500] [--candles 2000] [--rounds 5] \\
        [--out profiles/bbextreme_ab.txt]

  (i)   engine.bb_extreme_replay, every column: close and the three bands
        [S, T] in; status and the five value columns out
  (ii)  the same inputs, status only
  (iii) the staged composition that exists without the kernel: the gains and
        losses of close.diff() (one fused program), two exact rolling means
        (engine.rolling_many, the row-wide sequential replay), a rolling count
        of NaN closes, and one fused program for the RSI, evaluate's values
        and the gates. Its rolling sums start at the row's first candle, not
        at t - 29: the result is NOT the method's (the cells where its status
        differs from the kernel's are counted)
  (iv)  engine.buy_the_dip_replay, every column: the same mapping on 18 B in,
        25 B out per candle

The variants alternate within each round; HIP events time each call after
warm-up: a call's time holds its output allocations and whatever the host
takes to reach the launch. For the kernels' own time run this under a kernel
trace, in a run of its own. The bandwidth fraction counts each variant's
algorithmic bytes per candle against 8 TB/s: (i) 4 x 8 in, 1 + 5 x 8 out = 73;
(ii) 33; (iii) the differences 8 in and 16 out, the means 16 + 16, the NaN
flags and their count 8 + 8 + 8 + 8, the fused gate 7 x 8 in and 1 + 5 x 8
out = 185, a lower bound; (iv) 43.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine                          # noqa: E402
from binquant_amd import fused as F                     # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
STEP_MS = 900_000
P = engine.BB_EXTREME_DEFAULTS


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


def staged(c, up, mid, lo, tcol):
    """(iii): the gates of BBExtremeReversion.signal() from row-wide rolling means."""
    C = F.inp(c)
    d = C - F.shift(C, 1)
    gl = F.run({"gain": F.where(d > 0.0, d, 0.0), "loss": -F.where(d < 0.0, d, 0.0)})
    gain, loss = engine.rolling_many(engine.Roll(gl["gain"], P["rsi_window"]), engine.Roll(gl["loss"], P["rsi_window"]))
    nulls = engine.rolling(torch.isnan(c).to(torch.float64), P["lookback"], "isum", min_periods=1)
    G, Q, N, UP, MID, LO, TT = (F.inp(x) for x in (gain, loss, nulls, up, mid, lo, tcol))
    rsi = 100.0 - (100.0 / (1.0 + G / Q))
    clamped = F.where(rsi > 0.0, F.where(rsi < 100.0, rsi, 100.0), 0.0)
    span = UP - LO
    pos = F.where(span > 0.0, (C - LO) / span, 0.5)
    width = F.where(MID > 0.0, span / MID, 0.0)
    dist = F.where(MID > 0.0, (C - MID) / MID * 100.0, 0.0)
    buy = (clamped <= P["oversold_rsi"]) & (pos <= P["max_lower_band_position"])
    sell = (clamped >= P["overbought_rsi"]) & (pos >= P["min_upper_band_position"])
    code = F.const(0.0)
    for cond, value in reversed([(TT < float(P["lookback"] - 1), 2.0), (N > 0.0, 3.0), (rsi != rsi, 4.0),
                                 (span <= 0.0, 5.0), (~(buy | sell), 6.0)]):
        code = F.where(cond, value, code)
    return F.run({"status": code, "rsi_value": F.where(rsi != rsi, 50.0, clamped), "band_position": pos,
                  "bb_width": width, "distance_from_mid_pct": dist, "direction": F.where(buy, 0.0, 1.0)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, T = a.symbols, a.candles
    p = device_panel(S, T, seed=3)
    c = p["close"]
    mean, dev = engine.rolling(c, 20, "mean"), engine.rolling(c, 20, "std")
    up, mid, lo = mean + 1.5 * dev, mean, mean - 1.5 * dev
    del mean, dev
    g = torch.Generator(device="cuda").manual_seed(7)
    ct = (engine.BUY_THE_DIP_DEFAULTS["start_time_ms"] + STEP_MS * (torch.arange(T, device="cuda", dtype=torch.int64) + 1)
          - 1).expand(S, T).contiguous()
    mkt = torch.randint(-1, 5, (T,), device="cuda", generator=g).to(torch.int8)
    micro = torch.randint(-1, 5, (S, T), device="cuda", generator=g).to(torch.int8)
    tcol = torch.arange(T, device="cuda", dtype=torch.float64)

    status, _ = engine.bb_extreme_replay(c, up, mid, lo, columns=())
    st = staged(c, up, mid, lo, tcol)
    differ = int(st["status"].to(torch.uint8).ne(status).sum())
    counts = torch.bincount(status.flatten().to(torch.int64), minlength=7)
    summary = f"status 0..6 = {counts.tolist()}; cells where the staged status is not the kernel's: {differ}"
    del st, status

    variants = {
        "(i) replay, every column": lambda: engine.bb_extreme_replay(c, up, mid, lo),
        "(ii) replay, status only": lambda: engine.bb_extreme_replay(c, up, mid, lo, columns=()),
        "(iii) staged: 2 rolling means + count + gates": lambda: staged(c, up, mid, lo, tcol),
        "(iv) buy_the_dip_replay, every column": lambda: engine.buy_the_dip_replay(c, ct, mkt, micro),
    }
    nbytes = dict(zip(variants, (73, 33, 185, 43)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    lines = [f"bbextreme_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating", f"kernel: {S} x {T}; {summary}"]
    lines += table(timed(variants, a.rounds, a.warmup), note)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
