"""Timing of the liquidation-sweep gate and winner (bq_sweep.hip), in one
process: the kernel at the strategy rows' shape beside the pump pipeline that
produces its columns and a plain device copy, and the cohort as a replayed
graph with and without sweep=True.

    timeout -k 10 600 python tools/sweep_ab.py [--symbols 12500] [--candles 2000] [--rounds 3] \\
        [--cohort 1000x400] [--no-kernel] [--no-sweep] [--out profiles/sweep_ab.txt]

  (i)   engine.sweep_select over the 13 gate columns + score_cross + a route
        mask, every output (two launches: the gate / partial arg-max pass and
        the merge); the same without rank_score; and one column of it
        (t_range = the cohort's T - 2: the lane-per-row mapping)
  (ii)  strategies.pump_score_features (panel mode), the unchanged neighbour
        that writes those columns
  (iii) thirteen fp64 column copies (Tensor.copy_): what moving the same input
        bytes once costs in this run (the copy ceiling of DESIGN section 6)
  (iv)  cohort.process_cohort at the live shape as a replayed hipGraph, with
        and without sweep=True, alternating; --no-sweep times the default path
        only (the form that also runs on a tree without the feature, for the
        parent comparison)

The variants alternate within each round; HIP events time each call after
warm-up. The bandwidth fraction counts the select's algorithmic bytes
(13 x 8 + 2 in, 1 + 8 out per candle; 13 x 8 + 2 + 1 without rank_score)
against 8 TB/s; the copy moves 13 x 16 B per candle.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, strategies            # noqa: E402
from binquant_amd.cohort import process_cohort          # noqa: E402
from binquant_amd.graphs import CapturedPipeline        # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
SW_COLUMNS = ("pump_score", "score_threshold", "momentum_atr", "close", "prior_high", "close_location",
              "relative_volume", "volume_threshold", "trend_score", "ema20", "relative_strength", "btc_momentum_3",
              "btc_trend_score")


def timed(variants, rounds, warmup, reps=1):
    times = {k: [] for k in variants}
    for rnd in range(warmup + rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                res = fn()
            e1.record()
            e1.synchronize()
            del res
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) / reps)
    return times


def table(times, note=None):
    lines = [f"{'variant':44s} {'median ms':>10s} {'min':>8s} {'max':>8s}"]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{name:44s} {med:10.4f} {min(ts):8.4f} {max(ts):8.4f}  {note(name, med) if note else ''}")
    return lines


def kernel_part(S, T, rounds, warmup):
    p = device_panel(S, T, seed=3)
    o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
    btc = c[0].clone()
    pump = strategies.pump_score_features(o, h, l, c, v, btc)
    cols = [c if k == "close" else pump[k] for k in SW_COLUMNS]
    cross = pump["score_cross"]
    route = torch.rand(S, T, device="cuda") < 0.85
    status, _, winner, _ = engine.sweep_select(cols, cross, route_ok=route)
    counts = torch.bincount(status.flatten().to(torch.int64), minlength=256)
    summary = (f"status 0..14 = {counts[:15].tolist()}, no_frame = {int(counts[255])}, "
               f"columns with a winner = {int((winner >= 0).sum())} of {T}")
    del status, winner
    dst = [torch.empty_like(x) for x in cols]

    def copies():
        for d, s in zip(dst, cols):
            d.copy_(s)
        return dst[0]

    variants = {
        "sweep_select, every output": lambda: engine.sweep_select(cols, cross, route_ok=route),
        "sweep_select, no rank_score": lambda: engine.sweep_select(cols, cross, route_ok=route, rank_score=False),
        "sweep_select, one column (T - 2)": lambda: engine.sweep_select(cols, cross, route_ok=route,
                                                                        t_range=(T - 2, T - 1)),
        "pump_score_features (panel mode)": lambda: strategies.pump_score_features(o, h, l, c, v, btc),
        "13 fp64 column copies": copies,
    }
    nbytes = {"sweep_select, every output": 13 * 8 + 2 + 9, "sweep_select, no rank_score": 13 * 8 + 2 + 1,
              "13 fp64 column copies": 13 * 16}

    def note(name, med):
        if name not in nbytes:
            return ""
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    return [f"kernel: {S} x {T}; {summary}"] + table(timed(variants, rounds, warmup), note)


def cohort_part(S, T, rounds, warmup, with_sweep):
    p5, p15 = device_panel(S, T, seed=5), device_panel(S, T, seed=6)
    ts = 1_700_000_000_000 + 900_000 * torch.arange(T, device="cuda", dtype=torch.int64)
    ins = [p5[k] for k in ("open", "high", "low", "close", "volume")]
    ins += [p15[k] for k in ("open", "high", "low", "close", "volume")]
    ins += [ts.expand(S, T).contiguous(), ts, p15["close"][0].clone()]
    variants = {}
    plain = CapturedPipeline(process_cohort, *ins)
    variants["process_cohort graph, default"] = plain.graph.replay
    if with_sweep:
        route = torch.rand(S, device="cuda") < 0.85
        rank = torch.randperm(S, device="cuda").to(torch.int32)
        swept = CapturedPipeline(lambda *a: process_cohort(*a, sweep=True, sweep_route=route,
                                                           sweep_symbol_rank=rank), *ins)
        variants["process_cohort graph, sweep=True"] = swept.graph.replay
    times = timed(variants, rounds, warmup, reps=50)
    return [f"cohort: {S} x {T}, replayed graph, 50 replays per sample"] + table(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--cohort", default="1000x400")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"sweep_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating"]
    if not a.no_kernel:
        lines += kernel_part(a.symbols, a.candles, a.rounds, a.warmup)
    cs, ct = (int(x) for x in a.cohort.split("x"))
    lines += cohort_part(cs, ct, a.rounds, a.warmup, not a.no_sweep)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
