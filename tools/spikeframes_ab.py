"""Timing of the per-frame failed-spike pass (bq_spikeframes.hip), in one
process, beside what exists without it:

    timeout -k 10 600 python tools/spikeframes_ab.py [--shapes 1000x1000,12500x400] [--rounds 5] \\
        [--ends 16] [--trace] [--out profiles/spikeframes_ab.txt]

  (i)   strategies.failed_spike_frames, every column: the exact answer at
        every candle (the column stage, then bq_spike_frames' two kernels)
  (ii)  its column stage alone (strategies.spike_frame_columns: the close's
        ffill, the fused programs, one batched rolling call)
  (iii) engine.spike_frames alone on those columns: the expanding quantile
        and the flag / cooldown replay
  (iv)  (iii) with from_t = lens - 1: the live call (one column per row; the
        prefix is still inserted candle by candle)
  (v)   strategies.failed_spike_features over the whole row (panel mode): the
        approximation the pass replaces — right on each row's newest column
        only
  (vi)  the per-end route: failed_spike_features(panel[:, :t + 1], exact=True),
        timed at --ends evenly spaced ends t and extrapolated to one call per
        candle (the mean call time x T)

The variants alternate within each round; HIP events time each call after
warm-up, `reps` calls per sample so that a sample lasts ~0.2 s. --trace: run
(iii) a few times and nothing else, for a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/spikeframes_ab.py --trace):
the share of spike_prefix_quantile_kernel in (iii) comes from there.

--frame-cap M: the sliding frame cap (bq_spike_frames_capped) instead. (i) to
(iv) are the capped calls ((ii) with the two index columns), (i-u) / (iii-u) the
uncapped calls beside them where T <= engine.SPIKE_FRAMES_MAX_T, (vi) the
per-end route on the capped frames panel[:, max(0, t - M):t]. --panel dense
puts a qualifying spike every 5 candles on every row. Also printed: how many
cooldown walks evaluated rows of a slid frame's first 60 (the zone), counted
on the output's own label_pre column (a proxy: the kernel walks the labels
formed under each frame's thresholds)."""

from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from binquant_amd import engine, strategies             # noqa: E402
from binquant_amd.synth import device_panel             # noqa: E402


def sample(fn, reps: int) -> float:
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def reps_for(fn, target_ms: float = 200.0) -> int:
    fn()
    fn()
    torch.cuda.synchronize()
    one = max(sample(fn, 2), 1e-3)
    return max(2, min(200, int(target_ms / one)))


def zone_walks(label_pre: torch.Tensor, bars: int, cap: int) -> tuple[int, int]:
    """(labelled cells of slid frames, those whose walk back to the nearest run of `bars` clear rows ends inside
    the frame's first 60 rows), on one label_pre column per row."""
    S, T = label_pre.shape
    x = label_pre.to(torch.int32)
    cs = torch.cat([torch.zeros((S, 1), dtype=torch.int32, device=x.device), x.cumsum(1).to(torch.int32)], 1)
    j = torch.arange(T, device=x.device).reshape(1, T)
    lo = (j - bars).clamp(min=0)
    clear_before = ((cs[:, :T] - torch.gather(cs, 1, lo.expand(S, T))) == 0) & (j >= bars)   # rows j - bars .. j - 1
    start = torch.where(clear_before, j, torch.zeros_like(j)).cummax(1).values               # the walk's first row
    slid = label_pre & (j >= cap)
    return int(slid.sum()), int((slid & (start < j + 1 - cap + 60)).sum())


def dense_panel(p: dict) -> dict:
    """A bullish +3 % candle on 4x volume every 5 candles of every row."""
    c, v = p["close"].clone(), p["volume"].clone()
    T = c.shape[1]
    bump = torch.ones(T, dtype=c.dtype, device=c.device)
    bump[20::5] = 1.03
    c = c * bump.cumprod(0).reshape(1, T)
    v[:, 20::5] *= 4.0
    o = torch.cat([c[:, :1], c[:, :-1]], 1)
    return dict(open=o, high=torch.maximum(o, c) * 1.001, low=torch.minimum(o, c) * 0.999, close=c, volume=v)


def capped(a, lines: list[str]) -> None:
    par, M = strategies.SpikeParams(), a.frame_cap
    for shape in a.shapes.split(","):
        S, T = (int(x) for x in shape.split("x"))
        p = device_panel(S, T, seed=3)
        if a.panel == "dense":
            p = dense_panel(p)
        o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
        qv = v * c
        cols = strategies.spike_frame_columns(o, c, v, par, cap=True)
        live = torch.full((S,), T - 1, dtype=torch.int64, device="cuda")
        if a.trace:
            for _ in range(4):
                engine.spike_frames(cols, par, frame_cap=M)
            torch.cuda.synchronize()
            continue
        variants = {
            "(i) failed_spike_frames(frame_cap)": lambda: strategies.failed_spike_frames(o, h, l, c, v, qv, par,
                                                                                         frame_cap=M),
            "(ii) column stage with the index columns": lambda: strategies.spike_frame_columns(o, c, v, par, cap=True),
            "(iii) spike_frames(frame_cap) alone": lambda: engine.spike_frames(cols, par, frame_cap=M),
            "(iv) (iii) with from_t = lens - 1": lambda: engine.spike_frames(cols, par, from_t=live, frame_cap=M),
        }
        out = strategies.failed_spike_frames(o, h, l, c, v, qv, par, frame_cap=M)
        note = ""
        if T <= engine.SPIKE_FRAMES_MAX_T:
            variants["(i-u) failed_spike_frames, no cap"] = lambda: strategies.failed_spike_frames(o, h, l, c, v, qv, par)
            variants["(iii-u) spike_frames alone, no cap"] = lambda: engine.spike_frames(cols, par)
            plain = strategies.failed_spike_frames(o, h, l, c, v, qv, par)
            differs = sum(int((out[k] != plain[k]).sum()) for k in ("label", "price_break_flag",
                                                                    "cumulative_price_break_flag"))
            note = f"; cells where the uncapped answer differs in label / price_break / cumulative flag: {differs}"
        walks, in_zone = zone_walks(out["label_pre"], par.post_spike_cooldown_bars, M)
        lines.append(f"{S} x {T}, frame_cap {M}, {a.panel} panel: labels {int(out['label'].sum())} of "
                     f"{int(out['label_pre'].sum())} preliminary{note}; walks of slid frames {walks}, of them into "
                     f"the frame's first 60 rows {in_zone}")
        reps = {k: reps_for(fn) for k, fn in variants.items()}
        times: dict[str, list[float]] = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(sample(fn, reps[k]))
        lines.append(f"{'variant':44s} {'median ms':>10s} {'min':>8s} {'max':>8s}  reps")
        for k, ts in times.items():
            lines.append(f"{k:44s} {statistics.median(ts):10.4f} {min(ts):8.4f} {max(ts):8.4f}  {reps[k]}")
        ends = sorted({max(1, round((i + 1) * T / a.ends)) for i in range(a.ends)})
        per_end = []
        for t in ends:
            sl = [x[:, max(0, t - M):t].contiguous() for x in (o, h, l, c, v, qv)]
            fn = lambda: strategies.failed_spike_features(*sl, par, exact=True)   # noqa: E731
            fn()
            torch.cuda.synchronize()
            per_end.append(sample(fn, 3))
        mean = statistics.mean(per_end)
        first = statistics.median(times[list(variants)[0]])
        lines.append(f"{'(vi) per-end route, mean of ' + str(len(ends)) + ' ends':44s} {mean:10.4f} {min(per_end):8.4f} "
                     f"{max(per_end):8.4f}  x {T} candles = {mean * T:.1f} ms; (vi) x T / (i) = {mean * T / first:.0f}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame-cap", type=int, default=None)
    ap.add_argument("--panel", choices=("walk", "dense"), default="walk")
    ap.add_argument("--shapes", default="1000x1000,12500x400")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ends", type=int, default=16)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out")
    ap.add_argument("--stats", default=None, help="print the spike kernels' rows of a rocprofv3 kernel_stats.csv")
    a = ap.parse_args()
    if a.stats:
        import csv

        for r in csv.DictReader(open(a.stats)):
            if "spike" in r["Name"]:
                print(f"{r['Name'][:64]:64s} calls {r['Calls']:>4s} avg {float(r['AverageNs']) / 1e3:9.1f} us "
                      f"min {float(r['MinNs']) / 1e3:9.1f} max {float(r['MaxNs']) / 1e3:9.1f}")
        return
    lines = [f"spikeframes_ab on {torch.cuda.get_device_name(0)}, {a.rounds} rounds after warm-up, variants alternating"]
    par = strategies.SpikeParams()
    for shape in a.shapes.split(",") if a.frame_cap is None else ():
        S, T = (int(x) for x in shape.split("x"))
        p = device_panel(S, T, seed=3)
        o, h, l, c, v = (p[k] for k in ("open", "high", "low", "close", "volume"))
        qv = v * c
        cols = strategies.spike_frame_columns(o, c, v, par)
        live = torch.full((S,), T - 1, dtype=torch.int64, device="cuda")
        if a.trace:
            for _ in range(4):
                engine.spike_frames(cols, par)
            torch.cuda.synchronize()
            continue
        variants = {
            "(i) failed_spike_frames, every column": lambda: strategies.failed_spike_frames(o, h, l, c, v, qv, par),
            "(ii) column stage alone": lambda: strategies.spike_frame_columns(o, c, v, par),
            "(iii) spike_frames alone": lambda: engine.spike_frames(cols, par),
            "(iv) spike_frames, from_t = lens - 1": lambda: engine.spike_frames(cols, par, from_t=live),
            "(v) failed_spike_features, whole row": lambda: strategies.failed_spike_features(o, h, l, c, v, qv, par),
        }
        out = strategies.failed_spike_frames(o, h, l, c, v, qv, par)
        whole = strategies.failed_spike_features(o, h, l, c, v, qv, par, exact=True)
        differs = sum(int((out[k] != whole[k]).sum()) for k in ("label", "price_break_flag",
                                                                "cumulative_price_break_flag"))
        newest = all(bool((out[k][:, -1] == whole[k][:, -1]).all()) for k in engine._lib.SPIKE_FRAMES_OUT)
        lines.append(f"{S} x {T}: labels {int(out['label'].sum())} of {int(out['label_pre'].sum())} preliminary; "
                     f"cells where the whole-row pass differs in label / price_break / cumulative flag: {differs}; "
                     f"newest column equal: {newest}")
        reps = {k: reps_for(fn) for k, fn in variants.items()}
        times: dict[str, list[float]] = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(sample(fn, reps[k]))
        lines.append(f"{'variant':44s} {'median ms':>10s} {'min':>8s} {'max':>8s}  reps")
        for k, ts in times.items():
            lines.append(f"{k:44s} {statistics.median(ts):10.4f} {min(ts):8.4f} {max(ts):8.4f}  {reps[k]}")
        ends = sorted({max(1, round((i + 1) * T / a.ends)) for i in range(a.ends)})
        per_end = []
        for t in ends:
            sl = [x[:, :t].contiguous() for x in (o, h, l, c, v, qv)]
            fn = lambda: strategies.failed_spike_features(*sl, par, exact=True)   # noqa: E731
            fn()
            torch.cuda.synchronize()
            per_end.append(sample(fn, 3))
        mean = statistics.mean(per_end)
        lines.append(f"{'(vi) per-end route, mean of ' + str(len(ends)) + ' ends':44s} {mean:10.4f} {min(per_end):8.4f} "
                     f"{max(per_end):8.4f}  x {T} candles = {mean * T:.1f} ms")
        lines.append(f"(i) / (v) = {statistics.median(times[list(variants)[0]]) / statistics.median(times[list(variants)[4]]):.2f}; "
                     f"(vi) x T / (i) = {mean * T / statistics.median(times[list(variants)[0]]):.0f}")
    if a.frame_cap is not None:
        capped(a, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
