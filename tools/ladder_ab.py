"""Timing of the grid-ladder replay (bq_ladder.hip), in one process: the fused
pass at the strategy rows' shape beside the staged form that exists without
it and the frame scan alone.

    timeout -k 10 600 python tools/ladder_ab.py [--symbols 12500] [--candles 2000] [--rounds 5] \\
        [--out profiles/ladder_ab.txt]

  (i)   signals.grid_ladder_entry, every column, the bands the frame's own
        (bands=None: each band is read once)
  (i')  the same with the bands rounded by the caller (three more columns in)
  (ii)  signals.grid_ladder_entry, status only (columns=())
  (iii) the staged form available without the kernel: signals.bb_width_stable
        (stable and change_pct written out), then one fused element-wise
        program that reads them back with the close, the bands, the context
        and the snapshot and forms the status and the five values. This is
        the yardstick
  (iv)  signals.bb_width_stable alone: the floor for the frame scan

The context is per candle time ([T]: the grid-only policy's verdict, the
context's presence, its regime and long_regime_score, most of them passing),
the snapshot one entry per row ([S], the form a message cohort has). The
variants alternate within each round; HIP events time each call after
warm-up: a call's time holds its output allocations and whatever the host
takes to reach the launch. The bandwidth fraction counts each variant's
algorithmic bytes per candle against 8 TB/s: (i) close 8 and three bands 24 in,
status 1 and five values 40 out = 73; (i') 97; (ii) 33; (iii) the scan 24 in
and 9 out, the gate program 8 + 24 + 9 in and 41 out = 115; (iv) 33. The
verdict line compares (iii) - (i) with the spread the rounds themselves show
(the larger max - min of the two).
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import _lib, engine, signals          # noqa: E402
from binquant_amd import fused as F                     # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
P = engine.GRID_LADDER_DEFAULTS
RANGE = _lib.MARKET_REGIMES.index("RANGE")
NAN = float("nan")


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


def staged(c, up, md, lw, pok, cok, mk, score, sym):
    """(iii): LadderDeployer.signal()'s gates and values from bb_width_stable's outputs, one fused program."""
    S, T = c.shape
    bb = signals.bb_width_stable(up, md, lw, P["n"], P["max_change_pct"])
    C, U, M, L, ST, CH = (F.inp(x) for x in (c, up, md, lw, bb["stable"], bb["change_pct"]))
    POK, COK, MK, SC = F.inp(pok), F.inp(cok), F.inp(mk.to(torch.float64)), F.inp(score)
    row = lambda x: F.inp((x if x.dtype in (torch.bool, torch.float64) else x.to(torch.float64)).reshape(S, 1))   # noqa: E731
    SOK, SREG, STR, E20, E50, RS, ATR = (row(sym[k]) for k in signals.GL_SYM_KEYS)
    blocked = STR == float(_lib.MICRO_TRANSITIONS.index(signals.GL_BLOCKING_TRANSITIONS[0]))
    for name in signals.GL_BLOCKING_TRANSITIONS[1:]:
        blocked = blocked | (STR == float(_lib.MICRO_TRANSITIONS.index(name)))
    rw = F.where(M > 0.0, ((U - L) / M) * 100.0, 0.0)
    raw = (ATR * 100.0) * P["atr_multiplier"]
    low_side = F.where(raw < P["max_buffer_pct"], raw, P["max_buffer_pct"])      # min(4.0, raw)
    buf = F.where(low_side > P["min_buffer_pct"], low_side, P["min_buffer_pct"])   # max(0.5, ..)
    checks = [(~POK, 2.0), (~COK, 3.0), (MK != float(RANGE), 4.0), (~SOK | (SREG != float(RANGE)), 5.0),
              (blocked, 6.0), (~E20 & ~E50, 7.0), (RS <= 0.0, 8.0), (SC < P["min_long_score"], 9.0)]
    early = checks[0][0]
    for cond, _ in checks[1:]:
        early = early | cond
    f_price = ~((L < C) & (C < U))
    f_width = ~((rw >= P["min_width_pct"]) & (rw <= P["max_width_pct"]))
    checks += [(~ST, 10.0), (f_price, 11.0), (f_width, 12.0)]
    code = F.const(0.0)
    for cond, value in reversed(checks):
        code = F.where(cond, value, code)
    sized = ~early & ST & ~f_price
    emit = sized & ~f_width
    return F.run({"status": code, "bb_change_pct": F.where(~early, CH, NAN),
                  "range_width_pct": F.where(sized, rw, NAN), "breakout_buffer_pct": F.where(emit, buf, NAN),
                  "breakout_low": F.where(emit, L * (1.0 - buf / 100.0), NAN),
                  "breakout_high": F.where(emit, U * (1.0 + buf / 100.0), NAN)}, S, T)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, T = a.symbols, a.candles
    c = device_panel(S, T, seed=3)["close"]
    g = torch.Generator(device="cuda").manual_seed(7)
    # bands around the close: a half width of 1-4 % that drifts slowly, the close a little off the mid
    half = 0.01 + 0.03 * torch.rand((S, 1), device="cuda", generator=g, dtype=torch.float64)
    half = half * torch.exp(torch.cumsum(0.01 * torch.randn((S, T), device="cuda", generator=g, dtype=torch.float64), 1))
    md = c * (1.0 + 0.5 * half * (2.0 * torch.rand((S, T), device="cuda", generator=g, dtype=torch.float64) - 1.0))
    up, lw = md * (1.0 + half), md * (1.0 - half)
    del half
    rounded = tuple(torch.round(x * 1e6) / 1e6 for x in (up, md, lw))
    u = torch.rand(T, device="cuda", generator=g)
    pok, cok = u >= 0.03, u < 0.97
    mk = torch.where(torch.rand(T, device="cuda", generator=g) < 0.9, RANGE, 0).to(torch.int8)
    score = 0.15 + 0.7 * torch.rand(T, device="cuda", generator=g, dtype=torch.float64)
    ctx = torch.stack([mk.to(torch.float64), score])
    r = torch.rand((7, S), device="cuda", generator=g, dtype=torch.float64)
    sym = dict(ok=r[0] < 0.97, micro_regime=torch.where(r[1] < 0.93, RANGE, 3).to(torch.uint8),
               micro_transition=torch.where(r[2] < 0.8, _lib.MR_NONE, 2).to(torch.uint8), above_ema20=r[3] < 0.8,
               above_ema50=r[4] < 0.8, rs_vs_btc=r[5] - 0.08, atr_pct=0.04 * r[6])

    entry = lambda **kw: signals.grid_ladder_entry(c, up, md, lw, ctx, cok, pok, sym=sym, **kw)   # noqa: E731
    res = entry()
    st = staged(c, up, md, lw, pok, cok, mk, score, sym)
    torch.cuda.synchronize()
    differs = int(st["status"].to(torch.uint8).ne(res["status"]).sum())
    vdiff = {k: int((~((res[k] == st[k]) | (res[k].isnan() & st[k].isnan()))).sum()) for k in signals.GL_VALUES}
    counts = torch.bincount(res["status"].flatten().to(torch.int64), minlength=len(_lib.GL_REASONS))
    summary = (f"status 0..12 = {counts.tolist()}; cells where the staged status is not the kernel's: {differs}; "
               f"cells where a staged value is not: {vdiff}")
    del res, st

    variants = {
        "(i) fused, all columns": lambda: entry(),
        "(i') fused, all columns, rounded bands": lambda: entry(bands=rounded),
        "(ii) fused, status only": lambda: entry(columns=()),
        "(iii) staged: bb_width_stable + gate program": lambda: staged(c, up, md, lw, pok, cok, mk, score, sym),
        "(iv) bb_width_stable alone": lambda: signals.bb_width_stable(up, md, lw),
    }
    nbytes = dict(zip(variants, (73, 97, 33, 115, 33)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    times = timed(variants, a.rounds, a.warmup)
    names = list(variants)
    fused_t, staged_t = times[names[0]], times[names[3]]
    gain = statistics.median(staged_t) - statistics.median(fused_t)
    spread = max(max(fused_t) - min(fused_t), max(staged_t) - min(staged_t))
    lines = [f"ladder_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating", f"kernel: {S} x {T}; {summary}"]
    lines += table(times, note)
    lines.append(f"(iii) - (i) = {gain:.4f} ms against a run-to-run spread of {spread:.4f} ms: the fused pass is "
                 f"{'faster' if gain > spread else 'not faster'} than the staged form by more than the spread")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
