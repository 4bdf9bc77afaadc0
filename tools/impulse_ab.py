"""A/B timing of the entry-gate kernels (bq_impulse.hip) against the same
outputs composed from the staged entry points (engine.align, fused F
programs, a rolling integer sum), at the strategy rows' shape.

    python tools/impulse_ab.py [--symbols 12500] [--candles 2000] [--rounds 7] [--out profiles/impulse_ab.txt]

  (i)   signals.impulse_rider_features (one launch), all columns and status only
        against a benchmark with 1 % of its rows missing (the lookup's search
        path), and all columns against a complete benchmark (the guessed row)
  (ii)  the composition: two engine.align calls (the benchmark close, and the
        benchmark close four positions earlier, NaN for positions < 4) plus
        fused F programs for the stencil and the ordered gate
  (iii) signals.bb_width_stable against its composition (a fused program for
        the widths and bad rows, a rolling integer sum, a fused program for
        the change and the flag)

The compositions are first checked equal to the kernels (status exact, values
bit for bit) on the timed panel. The variants alternate within each round;
HIP events time each call after warm-up. Bandwidth fractions count the
algorithmic bytes (121 B per candle with every column, 49 B status only; 33 B
for bb_stable) against 8 TB/s.
"""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, signals   # noqa: E402
from binquant_amd import fused as F        # noqa: E402

NAN = float("nan")
PEAK = 8.0e12


def make_panel(S: int, T: int, seed: int = 1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *sh: torch.rand(*sh, device="cuda", dtype=torch.float64, generator=g)   # noqa: E731
    r = torch.randn(S, T, device="cuda", dtype=torch.float64, generator=g) * 0.005
    t = torch.arange(T, device="cuda")
    trig = ((t[None, :] + torch.randint(0, 23, (S, 1), device="cuda", generator=g)) % 23 == 0)
    r = torch.where(trig, torch.log1p(0.03 + 0.17 * rnd(S, T)), r)
    c = 10.0 ** (rnd(S, 1) * 5 - 2) * torch.exp(torch.cumsum(r, dim=1))
    o = torch.cat([c[:, :1], c[:, :-1]], dim=1)
    h = torch.maximum(o, c) * (1 + 0.002 * rnd(S, T))
    l = torch.minimum(o, c) * (1 - 0.002 * rnd(S, T))
    atr = c * (0.01 + 0.06 * rnd(S, T))
    c = torch.where(rnd(S, T) < 0.001, torch.full_like(c, NAN), c)
    grid = 1_760_400_000_000 + 900_000 * torch.arange(T, device="cuda", dtype=torch.int64)
    ts = grid.expand(S, T).contiguous()
    keep = rnd(T) > 0.01   # a benchmark with missing rows: both lookup paths
    bts = grid[keep].contiguous()
    bc = (60000.0 * torch.exp(torch.cumsum(torch.randn(T, device="cuda", dtype=torch.float64, generator=g) * 0.001,
                                           dim=0)))[keep].contiguous()
    return o, h, l, c, atr, ts, bts, bc


def composed_impulse(o, h, l, c, atr, ts, bts, bc, keys=signals.IR_KEYS, **thresholds):
    """signals.impulse_rider_features from the staged entry points."""
    P = {**engine.IMPULSE_DEFAULTS, **thresholds}
    S, T = c.shape
    bc4 = torch.cat([torch.full((4,), NAN, dtype=bc.dtype, device=bc.device), bc[:-4]])
    B, BA = F.inp(engine.align(ts, bts, bc)), F.inp(engine.align(ts, bts, bc4))
    C, O, H, L, A = (F.inp(x) for x in (c, o, h, l, atr))
    c_tr, o_tr, a_tr = F.shift(C, 1), F.shift(O, 1), F.shift(A, 1)
    a_imp, a_prev, c_pv = F.shift(C, 5), F.shift(C, 6), F.shift(C, 2)
    b_c, b_a = F.shift(B, 1), F.shift(BA, 1)
    fin = lambda x: ~F.isnan(x - x)   # noqa: E731
    ok = lambda x: (x > 0) & fin(x)   # noqa: E731
    impulse, previous, btc = c_tr / a_imp - 1, c_pv / a_prev - 1, b_c / b_a - 1
    rs, atr_pct, conf = impulse - btc, a_tr / c_tr, C / O - 1
    rng = H - L
    loc = (C - L) / rng
    tcol = torch.arange(T, device=c.device, dtype=torch.float64)
    checks = [
        F.inp(tcol) < float(P["min_history"] - 1),
        ~(ok(c_tr) & ok(o_tr) & ok(O) & ok(H) & ok(L) & ok(C) & ok(a_tr)),
        (a_imp <= 0) | (a_prev <= 0) | (c_pv <= 0),
        (b_a <= 0) | (b_c <= 0) | ~fin(btc),
        rng <= 0,
        ~(fin(impulse) & fin(previous) & fin(btc) & fin(rs) & fin(atr_pct) & fin(conf) & fin(loc)),
        ~((impulse >= P["min_impulse"]) & (impulse <= P["max_impulse"])),
        previous >= P["min_impulse"],
        btc > P["max_btc_return"],
        rs < P["min_rs"],
        atr_pct > P["max_atr_pct"],
        C < c_tr,
        conf < P["min_conf_return"],
        loc < P["min_close_location"],
    ]
    code = F.const(0.0)
    for i in range(len(checks), 0, -1):
        code = F.where(checks[i - 1], float(i), code)
    status_f = F.run({"status": code}, S, T)["status"]
    ex = dict(zip(signals.IR_KEYS, (impulse, previous, btc, rs, c_tr / o_tr - 1, conf, loc, atr_pct,
                                    C * P["entry_factor"])))
    ready = F.inp(status_f) == 0.0
    out = F.run({k: F.where(ready, ex[k], NAN) for k in keys}, S, T) if keys else {}
    return out, status_f.to(torch.uint8)


def composed_bb(up, mid, lw, n: int = 8, max_change: float = 20.0):
    S, T = mid.shape
    U, M, L = F.inp(up), F.inp(mid), F.inp(lw)
    W = (U - L) / M
    st = F.run({"w": W, "bad": F.where((M <= 0) | (W <= 0), 1.0, 0.0)}, S, T)
    (nbad,) = engine.rolling_many(engine.Roll(st["bad"], n, "isum", min_periods=n))
    Wt = F.inp(st["w"])
    w0 = F.shift(Wt, n - 1)
    change = ((Wt - w0) / w0).abs() * 100.0
    reached = F.inp(nbad) == 0.0
    return F.run({"stable": reached & (change <= max_change), "change_pct": F.where(reached, change, NAN)}, S, T)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype.is_floating_point:
        return bool(torch.equal(torch.nan_to_num(a, nan=-1.25e300).view(torch.int64),
                                torch.nan_to_num(b, nan=-1.25e300).view(torch.int64)))
    return bool(torch.equal(a, b))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=12500)
    ap.add_argument("--candles", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, T = a.symbols, a.candles
    o, h, l, c, atr, ts, bts, bc = make_panel(S, T)
    args = (o, h, l, c, atr, ts, bts, bc)
    mid = engine.rolling(c, 20, "mean")
    half = 2.0 * engine.rolling(c, 20, "std")
    up, lw = mid + half, mid - half
    del half

    # the compositions equal the kernels on the timed panel
    kv, ks = signals.impulse_rider_features(*args)
    cv, cs = composed_impulse(*args)
    assert same(ks, cs), "composition: status differs"
    for k in signals.IR_KEYS:
        assert same(kv[k], cv[k]), f"composition: {k} differs"
    confirmed = int((ks == 0).sum())
    kb, cb = signals.bb_width_stable(up, mid, lw), composed_bb(up, mid, lw)
    assert same(kb["stable"], cb["stable"]) and same(kb["change_pct"], cb["change_pct"]), "bb composition differs"
    del kv, ks, cv, cs, kb, cb

    grid = ts[0].contiguous()   # a complete benchmark frame: every lookup takes the guessed row
    gc = torch.zeros(T, dtype=torch.float64, device="cuda").index_copy_(0, torch.searchsorted(grid, bts), bc)
    gc = torch.where(gc == 0, gc.roll(1), gc)
    full = (o, h, l, c, atr, ts, grid, gc)
    variants = {
        "impulse kernel, complete benchmark": lambda: signals.impulse_rider_features(*full, check_bench=False),
        "impulse kernel, all columns": lambda: signals.impulse_rider_features(*args, check_bench=False),
        "impulse kernel, status only": lambda: signals.impulse_rider_features(*args, columns=(), check_bench=False),
        "impulse composition, all columns": lambda: composed_impulse(*args),
        "impulse composition, status only": lambda: composed_impulse(*args, keys=()),
        "bb_stable kernel": lambda: signals.bb_width_stable(up, mid, lw),
        "bb_stable composition": lambda: composed_bb(up, mid, lw),
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
    nbytes = {"impulse kernel, complete benchmark": 121, "impulse kernel, all columns": 121, "impulse kernel, status only": 49, "bb_stable kernel": 33}
    lines = [f"impulse_ab: {S} x {T} on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after {a.warmup} warm-up, "
             f"variants alternating; {confirmed} confirmed candles; compositions equal the kernels bit for bit",
             f"{'variant':36s} {'median ms':>10s} {'min':>8s} {'max':>8s}  fraction of 8 TB/s (algorithmic bytes)"]
    med = {}
    for name, ts_ in times.items():
        med[name] = statistics.median(ts_)
        frac = f"{nbytes[name] * S * T / (med[name] * 1e-3) / PEAK:.3f} at {nbytes[name]} B/candle" \
            if name in nbytes else ""
        lines.append(f"{name:36s} {med[name]:10.3f} {min(ts_):8.3f} {max(ts_):8.3f}  {frac}")
    for kern, comp in (("impulse kernel, all columns", "impulse composition, all columns"),
                       ("impulse kernel, status only", "impulse composition, status only"),
                       ("bb_stable kernel", "bb_stable composition")):
        faster = max(times[kern]) < min(times[comp])
        lines.append(f"{kern}: {med[comp] / med[kern]:.2f}x the composition's speed; slowest kernel round "
                     f"{max(times[kern]):.3f} ms {'<' if faster else '>='} fastest composition round "
                     f"{min(times[comp]):.3f} ms -> {'faster beyond the spread' if faster else 'NOT separated'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
