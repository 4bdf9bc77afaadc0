"""Timing of the buy-the-dip replay (bq_dip.hip), in one process: the kernel at
the strategy rows' shape beside the staged composition that exists without it
and the same-mapping price-tracker replay, and the cohort as a replayed graph
with and without buy_the_dip=.

    timeout -k 10 600 python tools/dip_ab.py [--symbols 12500] [--candles 2000] [--rounds 5] \\
        [--cohort 1000x400] [--no-kernel] [--no-cohort] [--no-feature] [--out profiles/dip_ab.txt]

  (i)   engine.buy_the_dip_replay, every column: close and close_time [S, T]
        in, the regimes' bytes, the EMA formed in the pass; status and the
        three value columns out
  (ii)  the same inputs, status only
  (iii) the staged composition that exists without the kernel: engine.ewm(c,
        span=20), torch.searchsorted of close_time - lookback_ms in each
        row's close_time plus a gather of close, the start-time comparison,
        and one fused program for the gates and change_6h (the regimes handed
        over as float64, converted outside the timed region). It has no null
        gate. On this gap-free panel without NaN its status must equal the
        kernel's cell for cell (asserted against the kernel fed the same ema20
        tensor)
  (iv)  engine.price_tracker_replay with trend_score given, every column: the
        same mapping on 80 B in, 50 B out per candle
  (v)   cohort.process_cohort at the live shape as a replayed hipGraph, default
        and with buy_the_dip=True, alternating; --no-feature times the default
        path only (the form that also runs on a tree without the feature, for
        the parent comparison)

The variants alternate within each round; HIP events time each call after
warm-up: a call's time holds its output allocations and whatever the host
takes to reach the launch. For the kernels' own time run the kernel part under
a kernel trace, in a run of its own (--no-cohort). The bandwidth fraction
counts each variant's algorithmic bytes per candle against 8 TB/s: (i) 8 + 8
in, the two regime bytes, 1 + 3 x 8 out = 43 (the probe's 24 B per lane come
from L2 and are not counted); (ii) 18 + 1 = 19; (iii) ewm 8 + 8, the target
and searchsorted 8 + 8 + 8 + 8, the index clamp and gather 8 + 8 + 8 + 8 + 8,
the start comparison 8 + 1, the fused program 8 x 5 + 2 in and 8 + 8 out =
165, a lower bound (searchsorted's probes re-read close_time); (iv) 130.
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
from binquant_amd.cohort import process_cohort          # noqa: E402
from binquant_amd.graphs import CapturedPipeline        # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
STEP_MS = 900_000
P = engine.BUY_THE_DIP_DEFAULTS


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


def staged(c, ct, mkt_f, micro_f, tcol):
    """(iii): the gates of BuyTheDip.signal() without the kernel (no null gate)."""
    ema = engine.ewm(c, span=float(P["ema_span"]))
    idx = torch.searchsorted(ct, ct - P["lookback_ms"], right=True) - 1   # the last candle at or before the target
    ref = c.gather(1, idx.clamp(min=0))
    found, started = idx >= 0, ct >= P["start_time_ms"]
    C, REF, EMA, MK, MR, TT = (F.inp(x) for x in (c, ref, ema, mkt_f, micro_f, tcol))
    change = F.where(REF == 0.0, 0.0, (C - REF) / REF.abs()) * 100.0
    blocked = (MK == 0.0) | (MK == 1.0) | (MR == 0.0) | (MR == 1.0)
    code = F.const(0.0)
    for cond, value in reversed([
            (TT < float(P["lookback_candles"] - 1), 2.0), (~F.inp(started), 3.0), (~F.inp(found), 4.0),
            ((change > P["max_change_pct"]) | (change <= P["min_change_pct"]), 5.0), (blocked, 6.0),
            (~((C > F.shift(C, 1)) & (C > EMA)), 7.0)]):
        code = F.where(cond, value, code)
    res = F.run({"status": code, "change_6h": change})
    res.update(reference_price=ref, ema20=ema)
    return res


def kernel_part(S, T, rounds, warmup):
    p = device_panel(S, T, seed=3)
    h, l, c, v = (p[k] for k in ("high", "low", "close", "volume"))
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    ct = (P["start_time_ms"] + STEP_MS * (torch.arange(T, device="cuda", dtype=torch.int64) + 1) - 1).expand(S, T) \
        .contiguous()
    mkt = torch.randint(-1, 5, (T,), device="cuda", generator=g).to(torch.int8)
    micro = torch.randint(-1, 5, (S, T), device="cuda", generator=g).to(torch.int8)
    mkt_f, micro_f = mkt.to(torch.float64), micro.to(torch.float64)
    tcol = torch.arange(T, device="cuda", dtype=torch.float64)

    st = staged(c, ct, mkt_f, micro_f, tcol)
    status, _ = engine.buy_the_dip_replay(c, ct, mkt, micro, ema20=st["ema20"], columns=())
    assert torch.equal(status, st["status"].to(torch.uint8)), "the staged status differs from the kernel's"
    own, _ = engine.buy_the_dip_replay(c, ct, mkt, micro, columns=())
    differ = int(own.ne(status).sum())
    counts = torch.bincount(own.flatten().to(torch.int64), minlength=8)
    summary = (f"status 0..7 = {counts.tolist()}; staged status == kernel's (ema20 shared): True; "
               f"cells where the in-pass EMA decides otherwise: {differ}")
    del st, status, own

    # (iv)'s inputs, as tools/pricetracker_ab.py draws them
    rsi, mfi = 5.0 + 60.0 * rnd(S, T), 2.0 + 46.0 * rnd(S, T)
    macd = 0.03 * (rnd(S, T) - 0.65)
    rs = 0.06 * (rnd(S, T) - 0.45)
    trend = 0.01 * (rnd(S, T) - 0.5)
    ctx = torch.stack([0.3 + 0.65 * rnd(T), 1.2 * rnd(T) - 0.6, 1.2 * rnd(T) - 0.5, 0.05 + 0.65 * rnd(T)])
    ctx_ok = rnd(T) > 0.08

    variants = {
        "(i) replay, every column": lambda: engine.buy_the_dip_replay(c, ct, mkt, micro),
        "(ii) replay, status only": lambda: engine.buy_the_dip_replay(c, ct, mkt, micro, columns=()),
        "(iii) staged: ewm + searchsorted + fused gates": lambda: staged(c, ct, mkt_f, micro_f, tcol),
        "(iv) price_tracker_replay, trend_score given": lambda: engine.price_tracker_replay(
            c, rsi, macd, mfi, ct, rs, ctx, ctx_ok, h=h, l=l, v=v, trend_score=trend),
    }
    nbytes = dict(zip(variants, (43, 19, 165, 130)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    return [f"kernel: {S} x {T}; {summary}"] + table(timed(variants, rounds, warmup), note)


def cohort_part(S, T, rounds, warmup, with_feature):
    p5, p15 = device_panel(S, T, seed=5), device_panel(S, T, seed=6)
    ts = P["start_time_ms"] + STEP_MS * torch.arange(T, device="cuda", dtype=torch.int64)
    ins = [p5[k] for k in ("open", "high", "low", "close", "volume")]
    ins += [p15[k] for k in ("open", "high", "low", "close", "volume")]
    ins += [ts.expand(S, T).contiguous(), ts, p15["close"][0].clone()]
    variants = {}
    plain = CapturedPipeline(process_cohort, *ins)
    variants["process_cohort graph, default"] = plain.graph.replay
    if with_feature:
        ct15 = (ts + STEP_MS - 1).expand(S, T).contiguous()
        mkt = torch.full((1,), 2, device="cuda", dtype=torch.int8)
        micro = torch.randint(-1, 5, (S,), device="cuda").to(torch.int8)
        dip = CapturedPipeline(lambda *a: process_cohort(*a, buy_the_dip=True, ct15=ct15, dip_regimes=(mkt, micro)),
                               *ins)
        variants["process_cohort graph, buy_the_dip"] = dip.graph.replay
    times = timed(variants, rounds, warmup, reps=50)
    return [f"cohort: {S} x {T}, replayed graph, 50 replays per sample"] + table(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--cohort", default="1000x400")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-cohort", action="store_true")
    ap.add_argument("--no-feature", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"dip_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating"]
    if not a.no_kernel:
        lines += kernel_part(a.symbols, a.candles, a.rounds, a.warmup)
    if not a.no_cohort:
        cs, ct = (int(x) for x in a.cohort.split("x"))
        lines += cohort_part(cs, ct, a.rounds, a.warmup, not a.no_feature)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
