"""Cost of the dense breadth at the live tick: engine.breadth_partial at S = 10 000, T = 1 (the last column,
row stride 64, of a 64-candle panel's features). Median over 7 batches of 200 calls, HIP events; the kernel is
~18 us, so the figure is bound by the host side of the call.

    python tools/breadth_tick_cost.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from binquant_amd import engine  # noqa: E402
from binquant_amd.synth import device_panel  # noqa: E402

S, T = 10_000, 64
p = device_panel(S, T, seed=99)
feats = engine.market_features(p["high"], p["low"], p["close"], max_bars=400)
c1 = p["close"][:, -1:]
f1 = {k: v[:, -1:] for k, v in feats.items()}
out = torch.empty((1, 10), dtype=torch.float64, device=c1.device)
for _ in range(20):
    engine.breadth_partial(c1, f1, out=out)
torch.cuda.synchronize()
assert out[0, 0].item() == S
ts = []
for _ in range(7):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        engine.breadth_partial(c1, f1, out=out)
    e.record()
    torch.cuda.synchronize()
    ts.append(a.elapsed_time(e) / 200)
print(f"breadth_tick {S}x1 ms/call {statistics.median(ts):.5f} min {min(ts):.5f} max {max(ts):.5f}", flush=True)
