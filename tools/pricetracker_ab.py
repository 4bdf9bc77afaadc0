"""Timing of the price-tracker replay (bq_pricetracker.hip), in one process: the
kernel at the strategy rows' shape beside the staged composition that exists
without it and the same-mapping spike-fade replay, and the cohort as a
replayed graph with and without price_tracker= / burst_entry=.

    timeout -k 10 600 python tools/pricetracker_ab.py [--symbols 12500] [--candles 2000] [--rounds 3] \\
        [--cohort 1000x400] [--no-kernel] [--no-feature] [--out profiles/pricetracker_ab.txt]

  (i)   engine.price_tracker_replay, every column: close, rsi, macd, mfi, high,
        low, volume, close_time and symbol_rs [S, T] in, the EMA formed in the
        pass; status, detail and the six value columns out
  (ii)  the same inputs, status only
  (iii) the same with trend_score given (one more column in), every column out
  (iv)  the staged lower bound that exists without the kernel:
        signals.trend_score(c, 9, 21) plus one fused expression set for the
        null gate, the oversold test, local_score, the LONG context score and
        the three rejections (the 192-instruction limit of a fused program
        splits its six outputs into two launches that re-read the columns).
        It has no cooldown and no close_time. On this gap-free
        panel its pass bit must equal the kernel's status not in {1, .., 5}
        (asserted against the kernel fed the same trend_score tensor)
  (v)   engine.spike_fade_replay, every output: the same mapping on 24 + 8 + 1 B
        in, 3 B out per candle
  (vi)  cohort.process_cohort at the live shape as a replayed hipGraph, default
        and with price_tracker= and burst_entry=True, alternating; --no-feature
        times the default path only (the form that also runs on a tree without
        the feature, for the parent comparison)

The variants alternate within each round; HIP events time each call after
warm-up. The bandwidth fraction counts each variant's algorithmic bytes per
candle against 8 TB/s: (i) nine 8-byte input columns + 2 + 6 x 8 out = 122;
(ii) 72 + 1 = 73; (iii) 80 + 50 = 130; (iv) 8 + 8 for trend_score, then nine
columns in once and the pass byte + five columns out = 129 (a lower bound:
the second launch re-reads seven of them); (v) 36. The context
rows ([4, T]) stay in L2 and are not counted.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, signals                # noqa: E402
from binquant_amd import fused as F                     # noqa: E402
from binquant_amd.cohort import process_cohort          # noqa: E402
from binquant_amd.graphs import CapturedPipeline        # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402

PEAK = 8.0e12
STEP_MS = 300_000


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


def _clamp(x, lo=-1.0, hi=1.0):
    m = F.where(x < hi, x, hi)
    return F.where(m > lo, m, lo)


def _nneg(x):
    return F.where(x > 0.0, x, 0.0)


def staged(c, rsi, macd, mfi, h, l, v, rs, ctx, ctx_ok, tcol):
    """(iv): the gates and scores of PriceTracker.signal() without the kernel."""
    trend = signals.trend_score(c, 9, 21)
    C, R, M, MF, H, L, V, RS, TR = (F.inp(x) for x in (c, rsi, macd, mfi, h, l, v, rs, trend))
    CONF, TAIL, BTC, STRESS = (F.inp(ctx[k]) for k in range(4))
    OK, TT = F.inp(ctx_ok), F.inp(tcol)
    # a NaN among the six columns of the last five rows: NaN propagates through a sum (the panel holds no
    # infinities, whose differences would also give NaN), which keeps the program within the instruction limit
    six = C + R + M + H + L + V
    tail = six
    for k in range(1, 5):
        tail = tail + F.shift(six, k)
    ready = (TT >= 29.0) & ~F.isnan(F.where(TT >= 4.0, tail, 0.0))
    setup = (R < 30.0) & (M < 0.0) & (MF < 20.0)
    local = ((1.0 + _nneg((30.0 - R) / 30.0) * 0.35) + _nneg((20.0 - MF) / 20.0) * 0.35) \
        + F.where(M.abs() * 100.0 > 1.0, 1.0, M.abs() * 100.0) * 0.3
    real = OK & ~(CONF <= 0.0)
    btc_al = _clamp(BTC)
    cross = _clamp(0.6 * RS + 0.4 * TR)
    over = _clamp(0.6 * _nneg(RS) + 0.4 * _nneg(TR), 0.0, 1.0)
    sup = _clamp(0.35 * TAIL + 0.25 * btc_al + 0.25 * cross + 0.15 * (-STRESS))
    fol = _clamp(0.45 * TAIL + 0.3 * btc_al + 0.25 * cross)
    adv = _clamp(0.55 * STRESS + 0.25 * _nneg(-sup) + 0.2 * (1.0 - over), 0.0, 1.0)
    boost = (TAIL < 0.0) & (over > 0.0)
    sup = F.where(boost, _clamp(sup + 0.2 * over), sup)
    fol = F.where(boost, _clamp(fol + 0.15 * over), fol)
    conf, fol, adv, sup = (F.where(real, x, 0.0) for x in (CONF, fol, adv, sup))
    adj = local + conf * 0.35 * (fol + (0.2 * sup) - (0.35 * adv))
    rej = (fol < -0.2) | (adv > 0.6) | (conf < 0.5)
    res = F.run({"pass": ready & setup & OK & ~rej, "local_score": local, "followthrough": fol, "adverse_risk": adv,
                 "supportiveness": sup, "adjusted_score": adj})
    res["trend_score"] = trend
    return res


def kernel_part(S, T, rounds, warmup):
    p = device_panel(S, T, seed=3)
    o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    rsi, mfi = 5.0 + 60.0 * rnd(S, T), 2.0 + 46.0 * rnd(S, T)
    macd = 0.03 * (rnd(S, T) - 0.65)
    rs = 0.06 * (rnd(S, T) - 0.45)
    ctx = torch.stack([0.3 + 0.65 * rnd(T), 1.2 * rnd(T) - 0.6, 1.2 * rnd(T) - 0.5, 0.05 + 0.65 * rnd(T)])
    ctx_ok = rnd(T) > 0.08
    ct = (1_700_000_000_000 + STEP_MS * (torch.arange(T, device="cuda", dtype=torch.int64) + 1) - 1).expand(S, T) \
        .contiguous()
    tcol = torch.arange(T, device="cuda", dtype=torch.float64)
    ts = ct - (STEP_MS - 1)
    src = torch.rand(S, T, device="cuda") < 0.05

    every = lambda **kw: engine.price_tracker_replay(c, rsi, macd, mfi, ct, rs, ctx, ctx_ok, h=h, l=l, v=v, **kw)   # noqa: E731
    st = staged(c, rsi, macd, mfi, h, l, v, rs, ctx, ctx_ok, tcol)
    status, _, _ = every(trend_score=st["trend_score"], columns=())
    kernel_pass = (status == 0) | (status == 6)
    assert torch.equal(kernel_pass, st["pass"]), "the staged pass bit differs from the kernel's"
    own, _, _ = every(columns=())
    differ = int(((own == 0) | (own == 6)).ne(kernel_pass).sum())
    counts = torch.bincount(own.flatten().to(torch.int64), minlength=7)
    summary = (f"status 0..6 = {counts.tolist()}; staged pass bit == kernel's (trend_score shared): True; "
               f"cells where the in-pass EMA decides otherwise: {differ}")
    trend = st["trend_score"]
    del st, status, own, kernel_pass

    variants = {
        "(i) replay, every column": lambda: every(),
        "(ii) replay, status only": lambda: every(detail=False, columns=()),
        "(iii) replay, trend_score given": lambda: every(trend_score=trend),
        "(iv) staged: trend_score + fused gate/score": lambda: staged(c, rsi, macd, mfi, h, l, v, rs, ctx, ctx_ok,
                                                                        tcol),
        "(v) spike_fade_replay, every output": lambda: engine.spike_fade_replay(o, h, c, ts, src),
    }
    nbytes = dict(zip(variants, (122, 73, 130, 16 + 129, 36)))

    def note(name, med):
        return f"{nbytes[name] * S * T / (med * 1e-3) / PEAK:.3f} of 8 TB/s at {nbytes[name]} B/candle"

    return [f"kernel: {S} x {T}; {summary}"] + table(timed(variants, rounds, warmup), note)


def cohort_part(S, T, rounds, warmup, with_feature):
    p5, p15 = device_panel(S, T, seed=5), device_panel(S, T, seed=6)
    ts = 1_700_000_000_000 + 900_000 * torch.arange(T, device="cuda", dtype=torch.int64)
    ins = [p5[k] for k in ("open", "high", "low", "close", "volume")]
    ins += [p15[k] for k in ("open", "high", "low", "close", "volume")]
    ins += [ts.expand(S, T).contiguous(), ts, p15["close"][0].clone()]
    variants = {}
    plain = CapturedPipeline(process_cohort, *ins)
    variants["process_cohort graph, default"] = plain.graph.replay
    if with_feature:
        ct5 = (1_700_000_000_000 + STEP_MS * (torch.arange(T, device="cuda", dtype=torch.int64) + 1) - 1) \
            .expand(S, T).contiguous()
        ctx = torch.tensor([[0.9], [0.4], [0.3], [0.1]], device="cuda", dtype=torch.float64)
        ok = torch.ones(1, device="cuda", dtype=torch.bool)
        rs = 0.02 * torch.randn(S, device="cuda", dtype=torch.float64)
        route = torch.rand(S, device="cuda") < 0.7
        state = signals.PriceTrackerState.empty(S, "cuda")
        both = CapturedPipeline(lambda *a: process_cohort(*a, price_tracker=state, ct5=ct5,
                                                          price_tracker_ctx=(ctx, ok), price_tracker_rs=rs,
                                                          burst_entry=True, burst_route=route), *ins)
        variants["process_cohort graph, price_tracker + burst"] = both.graph.replay
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
    ap.add_argument("--no-feature", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"pricetracker_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating"]
    if not a.no_kernel:
        lines += kernel_part(a.symbols, a.candles, a.rounds, a.warmup)
    cs, ct = (int(x) for x in a.cohort.split("x"))
    lines += cohort_part(cs, ct, a.rounds, a.warmup, not a.no_feature)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
