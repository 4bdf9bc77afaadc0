"""A/B timing of the five wave-per-row replay entry points whose device code
moved (csrc/bq_replay.h) between two builds of the library, at the shape the
tools/*_ab.py scripts of the five time (12 500 x 2 000, device_panel seed 3).

    python tools/replay_ab.py --parent <parent's libbinquant_amd.so> [--head <library>] \\
        [--rounds 5] [--out profiles/replay_ab.txt]

Each measurement is a fresh child process (its library chosen with
BQ_LIB_PATH) that builds the inputs, warms every entry point up and reports the
median HIP-event time of `--iters` calls through the engine wrapper, so the
wrappers' host work is inside the figure. Per round three children run one
after the other on the same device: the parent's library, the head's, the
parent's again (series P1, H, P2). One warm-up round is dropped.

The margin is what the parent shows against itself (tools/rowtile_ab.py): with
mP the median of all parent children (P1 and P2 pooled), the spread is the
largest |child - mP| over those children. The head's median over its rounds
must not exceed mP + spread (VERDICT within); below mP - spread it is
reported faster.

Rows, each entry point in its heaviest configuration (features formed in the
pass, per-candle context and snapshot, state, every column): retest,
spike_fade, price_tracker, mean_reversion, range_fade; and
price_tracker_trend (trend_score given, no high / low / volume) as the
lightest.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
ROWS = ("retest", "spike_fade", "price_tracker", "price_tracker_trend", "mean_reversion", "range_fade")
STEP_MS = 900_000


def child(S: int, T: int, iters: int, warmup: int) -> None:
    import torch

    sys.path.insert(0, str(ROOT))
    from binquant_amd import engine
    from binquant_amd.synth import device_panel

    p = device_panel(S, T, device="cuda", seed=3)
    o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    u8 = lambda x: x.to(torch.uint8)   # noqa: E731
    ot = (1_700_000_000_000 + STEP_MS * torch.arange(T, device="cuda", dtype=torch.int64)).expand(S, T).contiguous()
    ema, atr = c * (0.99 + 0.02 * rnd(S, T)), c * 0.0035 * (0.9 + 0.2 * rnd(S, T))
    bbm = c * (0.998 + 0.004 * rnd(S, T))
    bbu, bbl = bbm * 1.01, bbm * 0.99
    rsi, macd, mfi = 10 + 60 * rnd(S, T), -0.01 * rnd(S, T), 3 + 30 * rnd(S, T)
    leader, risk, source = rnd(S, T) < 0.06, rnd(S, T) < 0.6, rnd(S, T) < 0.05
    smk, fmk = rnd(S, T) < 0.9, rnd(S, T) < 0.5
    ctx = torch.stack([rnd(T) for _ in range(5)])
    ctx_ok = rnd(T) > 0.08
    rf_ctx = torch.stack([torch.zeros(T, device="cuda", dtype=torch.float64), 0.3 * rnd(T),
                          torch.full((T,), 2.0, device="cuda", dtype=torch.float64)])
    kind = u8(5 * rnd(S, T))
    mr_sym = (kind != 0, 0.004 + 0.03 * rnd(S, T), 0.01 * (rnd(S, T) - 0.6), u8(torch.where(kind == 4, 0, 2)),
              u8(torch.where(kind == 3, 1, 255)))
    rf_sym = (kind != 0, torch.full((S, T), 2, device="cuda", dtype=torch.uint8), u8(torch.where(kind == 3, 1, 255)),
              0.004 + 0.03 * rnd(S, T), 0.01 + 0.06 * rnd(S, T))
    rs, trend = 0.03 * (rnd(S, T) - 0.5), 0.03 * rnd(S, T)
    z8, z64 = (lambda: torch.zeros(S, dtype=torch.uint8, device="cuda")), (lambda: torch.zeros(S, dtype=torch.int64,
                                                                                             device="cuda"))
    nanf = lambda: torch.full((S,), float("nan"), dtype=torch.float64, device="cuda")   # noqa: E731
    calls = {
        "retest": lambda: engine.retest_replay(o, h, l, c, ema, ot, leader, risk, state=(z8(), z64(), nanf())),
        "spike_fade": lambda: engine.spike_fade_replay(o, h, c, ot, source, smk, fmk,
                                                       state=(z8(), z64(), nanf(), nanf())),
        "price_tracker": lambda: engine.price_tracker_replay(c, rsi, macd, mfi, ot, rs, ctx[:4], ctx_ok, h=h, l=l, v=v,
                                                             state=(z8(), z64())),
        "price_tracker_trend": lambda: engine.price_tracker_replay(c, rsi, macd, mfi, ot, rs, ctx[:4], ctx_ok,
                                                                   trend_score=trend, state=(z8(), z64())),
        "mean_reversion": lambda: engine.mean_reversion_replay(o, h, l, c, v, atr, bbu, ot, ctx, ctx_ok, sym=mr_sym,
                                                               state=(z8(), z64())),
        "range_fade": lambda: engine.range_fade_replay(o, h, l, c, v, rsi, bbu, bbm, bbl, rf_ctx, ctx_ok, sym=rf_sym),
    }
    res = {}
    for name in ROWS:
        fn, ts = calls[name], []
        for i in range(warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            del r
            if i >= warmup:
                ts.append(e0.elapsed_time(e1))
        res[name] = statistics.median(ts)
    print("REPLAY_AB " + json.dumps(res), flush=True)


def run_child(lib: str, a) -> dict[str, float]:
    env = dict(os.environ, BQ_LIB_PATH=str(Path(lib).resolve()))
    cmd = [sys.executable, __file__, "--child", "--symbols", str(a.symbols), "--candles", str(a.candles),
           "--iters", str(a.iters), "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=a.child_timeout).stdout
    line = [x for x in out.splitlines() if x.startswith("REPLAY_AB ")][-1]
    return json.loads(line[len("REPLAY_AB "):])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="library built from the parent commit")
    ap.add_argument("--head", default=str(ROOT / "binquant_amd" / "lib" / "libbinquant_amd.so"))
    ap.add_argument("--symbols", type=int, default=12_500)
    ap.add_argument("--candles", type=int, default=2_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.symbols, a.candles, a.iters, a.warmup)
        return 0
    if not a.parent or a.rounds < 5:
        ap.error("--parent is required, and at least 5 rounds")
    series = {"P1": [], "H": [], "P2": []}
    for rnd in range(1 + a.rounds):   # round 0: warm-up (file cache, clocks), dropped
        for key, lib in (("P1", a.parent), ("H", a.head), ("P2", a.parent)):
            r = run_child(lib, a)
            print(f"round {rnd} {key}: " + " ".join(f"{r[n]:.4f}" for n in ROWS), file=sys.stderr, flush=True)
            if rnd:
                series[key].append(r)
    lines = [f"replay_ab: {a.symbols} x {a.candles}, {a.rounds} rounds after 1 warm-up round; per round three fresh "
             f"processes alternate (parent, head, parent), each the median of {a.iters} calls after {a.warmup}; ms",
             f"{'row':20s} {'parent mP':>10s} {'P1 med':>8s} {'P2 med':>8s} {'spread':>8s} {'head':>8s} "
             f"{'head-mP':>8s}  verdict"]
    ok = True
    for name in ROWS:
        p1, p2, hd = ([r[name] for r in series[k]] for k in ("P1", "P2", "H"))
        mp = statistics.median(p1 + p2)
        spread = max(abs(x - mp) for x in p1 + p2)
        mh = statistics.median(hd)
        verdict = "within" if abs(mh - mp) <= spread else ("faster" if mh < mp else "SLOWER")
        ok &= verdict != "SLOWER"
        lines.append(f"{name:20s} {mp:10.4f} {statistics.median(p1):8.4f} {statistics.median(p2):8.4f} "
                     f"{spread:8.4f} {mh:8.4f} {mh - mp:+8.4f}  {verdict}")
        lines.append(f"{'':20s} P1 {' '.join(f'{x:.4f}' for x in p1)} | H {' '.join(f'{x:.4f}' for x in hd)} | "
                     f"P2 {' '.join(f'{x:.4f}' for x in p2)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
