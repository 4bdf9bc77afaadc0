"""Timing of the RS-reversal replay (bq_rsreversal.hip), in one process: the
kernel at the strategy rows' shape under three contexts, beside the staged
composition that exists without it and the same-mapping buy-the-dip replay.

    timeout -k 10 600 python tools/rsreversal_ab.py [--symbols 12500] [--candles 2000] [--rounds 5] \\
        [--out profiles/rsreversal_ab.txt]

  (i)   engine.rs_reversal_replay under a context that lets no candle through
        (TREND_UP at every candle time): the gates alone, no step sorts
  (ii)  a context of the fixture's kinds and limits
        (tests/golden/rsreversal_panel_gen.py) with other shares: drawn per run
        of 32-160 candle times, as regimes last, RANGE in 22 % of the runs (the
        fixture: 62 % of the candle times) and a weak RANGE market in about one
        run in seven; relative strength per cell with the fixture's shares. A
        small share of the 64-candle steps sorts (printed)
  (iii) every candle through: every step past the frame gate sorts
  (iv)  the staged composition that exists without the kernel:
        engine.rolling(volume, 96, "quantile", 0.2, min_periods=1) for every
        candle of every row, then one fused program for the gates. Its floor
        is pandas' rolling quantile, NOT the method's Series.quantile: the
        cells where its status or floor differs from the kernel's under (ii)'s
        context are counted
  (v)   engine.buy_the_dip_replay, every column: the same mapping on 18 B in,
        25 B out per candle

The variants alternate within each round; HIP events time each call after
warm-up: a call's time holds its output allocations and whatever the host
takes to reach the launch. For the kernels' own time run this under a kernel
trace, in a run of its own. The bandwidth fraction counts each variant's
algorithmic bytes per candle against 8 TB/s: (i)-(iii) volume 8, features_ok 1
and rs 8 in, status 1 and the floor 8 out = 26 (the context is [T]; the union
re-read of a sorting pair of steps, 8 x (window + 127) / 128 = 14 B a candle,
is not counted);
(iv) the rolling quantile 8 + 8, the gate 8 + 8 + 1 + 8 in and 1 + 8 out = 50;
(v) 43.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import _lib, engine                   # noqa: E402
from binquant_amd import fused as F                     # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
STEP_MS = 900_000
P = engine.RS_REVERSAL_DEFAULTS
RANGE = _lib.MARKET_REGIMES.index("RANGE")


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


def fixture_like_context(T):
    """context_ok, market_regime, average_return [T]: the fixture's kinds and limits, drawn per run of candle times."""
    cpu = torch.Generator().manual_seed(11)
    ok, mk, ar = torch.ones(T, dtype=torch.bool), torch.zeros(T, dtype=torch.int8), torch.zeros(T, dtype=torch.float64)
    kinds = torch.tensor([0.06, 0.06, 0.22, 0.2, 0.2, 0.13, 0.13])   # none, regime None, RANGE, the four others
    codes = (-1, -1, RANGE, 0, 1, 3, 4)
    t = 0
    while t < T:
        n = int(torch.randint(32, 161, (1,), generator=cpu))
        k = int(torch.multinomial(kinds, 1, generator=cpu))
        u = float(torch.rand(1, generator=cpu))
        ok[t:t + n], mk[t:t + n] = k != 0, codes[k]
        ar[t:t + n] = (-0.02 - 0.06 * u) if u < 0.7 else (P["avg_return_max"] if u < 0.76 else
                                                         float("nan") if u < 0.82 else 0.01)
        t += n
    return ok.cuda(), mk.cuda(), ar.cuda()


def staged(v, ok, mk, ar, fok, rs, tcol):
    """(iv): the gates of RelativeStrengthReversalRange.signal() from a row-wide rolling quantile."""
    floor = engine.rolling(v, P["window"], "quantile", P["quantile"], min_periods=1)
    V, FL, OK, MK, AR, FOK, RS, TT = (F.inp(x) for x in (v, floor, ok, mk.to(torch.float64), ar, fok, rs, tcol))
    code = F.const(0.0)
    for cond, value in reversed([(TT < float(P["window"] - 1), 2.0), (~OK, 3.0), (MK < 0.0, 4.0),
                                 (MK != float(RANGE), 5.0), (AR >= P["avg_return_max"], 6.0), (~FOK, 7.0),
                                 (RS <= P["rs_min"], 8.0), (V <= FL, 9.0)]):
        code = F.where(cond, value, code)
    return F.run({"status": code, "volume_floor": FL}, *v.shape)


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
    c, v = p["close"], torch.round(p["volume"] * 10.0) / 10.0
    del p
    g = torch.Generator(device="cuda").manual_seed(7)
    v[torch.rand((S, T), device="cuda", generator=g) < 0.005] = float("nan")   # missing candles: windows of 93-95 values
    u = torch.rand((S, T), device="cuda", generator=g, dtype=torch.float64)
    rs = torch.where(u < 0.60, 0.0501 + 0.35 * u, -0.3 + 0.35 * u)      # the fixture's shares: 60 % lead, 4 % at the
    rs = torch.where((u >= 0.60) & (u < 0.64), torch.full_like(rs, P["rs_min"]), rs)   # limit, 5 % NaN
    rs = torch.where((u >= 0.64) & (u < 0.69), torch.full_like(rs, float("nan")), rs)
    fok = (torch.arange(S, device="cuda") % 6 != 4)[:, None].expand(S, T).contiguous()
    del u
    lead = torch.full((S, T), 0.2, dtype=torch.float64, device="cuda")
    every = torch.ones((S, T), dtype=torch.bool, device="cuda")
    ctx_none = (torch.ones(T, dtype=torch.bool, device="cuda"), torch.zeros(T, dtype=torch.int8, device="cuda"),
                torch.full((T,), -0.05, dtype=torch.float64, device="cuda"))
    ctx_all = (ctx_none[0], torch.full((T,), RANGE, dtype=torch.int8, device="cuda"), ctx_none[2])
    ctx_fix = fixture_like_context(T)
    ct = (engine.BUY_THE_DIP_DEFAULTS["start_time_ms"] + STEP_MS * (torch.arange(T, device="cuda", dtype=torch.int64) + 1)
          - 1).expand(S, T).contiguous()
    mkt = torch.randint(-1, 5, (T,), device="cuda", generator=g).to(torch.int8)
    micro = torch.randint(-1, 5, (S, T), device="cuda", generator=g).to(torch.int8)
    tcol = torch.arange(T, device="cuda", dtype=torch.float64)

    status, vals = engine.rs_reversal_replay(v, *ctx_fix, fok, rs)
    st = staged(v, *ctx_fix, fok, rs, tcol)
    reached = (status == 0) | (status == 9)
    steps = torch.nn.functional.pad(reached.to(torch.uint8), (0, -T % 64)).reshape(S, -1, 64).any(dim=2)
    st_differs = int(st["status"].to(torch.uint8).ne(status).sum())
    a_, b_ = vals["volume_floor"][reached], st["volume_floor"][reached]
    fl_differs = int((~((a_ == b_) | (a_.isnan() & b_.isnan()))).sum())
    counts = torch.bincount(status.flatten().to(torch.int64), minlength=10)
    summary = (f"(ii): status 0..9 = {counts.tolist()}; reached {int(reached.sum())} of {S * T} cells "
               f"({reached.double().mean().item():.4f}), sorting steps {int(steps.sum())} of {steps.numel()} "
               f"({steps.double().mean().item():.4f}); cells where the staged status is not the kernel's: {st_differs}, "
               f"reached cells where its floor is not: {fl_differs}")
    del st, status, vals, reached, steps, a_, b_

    variants = {
        "(i) replay, no candle through": lambda: engine.rs_reversal_replay(v, *ctx_none, fok, rs),
        "(ii) replay, the fixture's context in runs": lambda: engine.rs_reversal_replay(v, *ctx_fix, fok, rs),
        "(iii) replay, every candle through": lambda: engine.rs_reversal_replay(v, *ctx_all, every, lead),
        "(iv) staged: rolling quantile + gates": lambda: staged(v, *ctx_fix, fok, rs, tcol),
        "(v) buy_the_dip_replay, every column": lambda: engine.buy_the_dip_replay(c, ct, mkt, micro),
    }
    nbytes = dict(zip(variants, (26, 26, 26, 50, 43)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    lines = [f"rsreversal_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating", f"kernel: {S} x {T}; {summary}"]
    lines += table(timed(variants, a.rounds, a.warmup), note)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
