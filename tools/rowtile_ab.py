"""A/B timing of the row-tile entry points whose device code moved
(csrc/bq_rowtile.h) between two builds of the library, at the shape bench.py
times its rows (12 500 x 2 000, device_panel seed 99).

    python tools/rowtile_ab.py --parent <parent's libbinquant_amd.so> [--head <library>] \\
        [--rounds 5] [--out profiles/rowtile_ab.txt]

Each measurement is a fresh child process (its library chosen with
BQ_LIB_PATH) that builds the panel, warms every entry point up and reports the
median HIP-event time of `--iters` calls. Per round three children run one
after the other on the same device: the parent's library, the head's, the
parent's again (series P1, H, P2). One warm-up round is dropped.

The margin is what the parent shows against itself: with mP the median of all
parent children (P1 and P2 pooled), the spread is the largest |child - mP| over
those children. The head's median over its rounds must not exceed mP + spread
(VERDICT within); below mP - spread it is reported faster.

Rows: a19_failed_spike (strategies.failed_spike_features, the spike walk) and
its base pass alone (engine.spike_base_std), a20_zscore, a20_adx,
a20_wilder_rsi, a11_beta_corr (the benchmark pre-pass and the symbol walk).
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
ROWS = ("a19_failed_spike", "spike_base_std", "a20_zscore", "a20_adx", "a20_wilder_rsi", "a11_beta_corr")


def child(S: int, T: int, iters: int, warmup: int) -> None:
    import torch

    sys.path.insert(0, str(ROOT))
    from binquant_amd import engine, signals, strategies
    from binquant_amd.synth import device_panel

    p = device_panel(S, T, device="cuda", seed=99)
    o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
    qv = v * c
    btc = c[0].clone()
    (cf,) = engine.rolling_many(engine.Ffill(c))
    calls = {
        "a19_failed_spike": lambda: strategies.failed_spike_features(o, h, l, c, v, qv),
        "spike_base_std": lambda: engine.spike_base_std(o, h, l, c, v, qv, cf),
        "a20_zscore": lambda: signals.zscore(c),
        "a20_adx": lambda: signals.adx(h, l, c),
        "a20_wilder_rsi": lambda: signals.wilder_rsi(c),
        "a11_beta_corr": lambda: engine.beta_corr(c, btc, 50),
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
    print("ROWTILE_AB " + json.dumps(res), flush=True)


def run_child(lib: str, a) -> dict[str, float]:
    env = dict(os.environ, BQ_LIB_PATH=str(Path(lib).resolve()))
    cmd = [sys.executable, __file__, "--child", "--symbols", str(a.symbols), "--candles", str(a.candles),
           "--iters", str(a.iters), "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=a.child_timeout).stdout
    line = [x for x in out.splitlines() if x.startswith("ROWTILE_AB ")][-1]
    return json.loads(line[len("ROWTILE_AB "):])


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
    lines = [f"rowtile_ab: {a.symbols} x {a.candles}, {a.rounds} rounds after 1 warm-up round; per round three fresh "
             f"processes alternate (parent, head, parent), each the median of {a.iters} calls after {a.warmup}; ms",
             f"{'row':18s} {'parent mP':>10s} {'P1 med':>8s} {'P2 med':>8s} {'spread':>8s} {'head':>8s} "
             f"{'head-mP':>8s}  verdict"]
    ok = True
    for name in ROWS:
        p1, p2, hd = ([r[name] for r in series[k]] for k in ("P1", "P2", "H"))
        mp = statistics.median(p1 + p2)
        spread = max(abs(x - mp) for x in p1 + p2)
        mh = statistics.median(hd)
        verdict = "within" if abs(mh - mp) <= spread else ("faster" if mh < mp else "SLOWER")
        ok &= verdict != "SLOWER"
        lines.append(f"{name:18s} {mp:10.4f} {statistics.median(p1):8.4f} {statistics.median(p2):8.4f} "
                     f"{spread:8.4f} {mh:8.4f} {mh - mp:+8.4f}  {verdict}")
        lines.append(f"{'':18s} P1 {' '.join(f'{x:.4f}' for x in p1)} | H {' '.join(f'{x:.4f}' for x in hd)} | "
                     f"P2 {' '.join(f'{x:.4f}' for x in p2)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
