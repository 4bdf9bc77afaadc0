"""bench.py --gpus N starts N ranks by itself: the driver
may run `python bench.py --gpus N` without torch.distributed.run. The rank
count must equal --gpus, or the run fails (rc != 0) instead of timing one
rank labelled as N."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _bench(args, env_extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_world_mismatch_fails_before_any_gpu_call():
    r = _bench(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, 120)
    assert r.returncode != 0
    assert "--gpus 4 but the launcher started 2 rank(s)" in r.stderr


def test_failing_rank_ends_the_run():
    """a rank that exits non-zero at start-up (here rank 1, by the
    BQ_BENCH_FAIL_RANK test hook) must end the self-launched run with its
    code; rank 0, left waiting in the gloo rendezvous for it, is stopped by
    the parent instead of hanging until the process-group timeout."""
    import time

    t0 = time.perf_counter()
    r = _bench(["--gpus", "2"], {"BQ_BENCH_BACKEND": "gloo", "BQ_BENCH_FAIL_RANK": "1:7",
                                 "BQ_BENCH_PG_TIMEOUT": "300"}, 200)
    assert r.returncode == 7, (r.returncode, r.stderr[-2000:])
    assert "the other ranks were stopped" in r.stderr
    assert time.perf_counter() - t0 < 150


@pytest.mark.gpu
def test_bench_gpus_2_self_launch_gloo(cuda):
    """On the one-GPU box: `BQ_BENCH_BACKEND=gloo bench.py --gpus 2` (two
    ranks sharing the GPU, collectives over gloo) reports n_gpus 2, the
    whole panel's symbols, the breadth leg's tracked total from the one
    all-reduce equal to every symbol of both shards, and the CPU baseline
    (rank 0, at every world size) present."""
    S, T = 3000, 512
    r = _bench(["--gpus", "2", "--symbols", str(S), "--candles", str(T), "--steps", "2", "--warmup", "1",
                "--full", "--no-shard", "--no-tick", "--no-rows", "--breadth-steps", "1",
                "--cpu-seconds", "1", "--cpu-workers", "2"],
               {"BQ_BENCH_BACKEND": "gloo"}, 240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2
    assert res["config"]["symbols"] == S and res["config"]["symbols_per_gpu"] == S // 2
    assert res["breadth"]["tracked_symbols"] == S
    assert res["value"] > 0
    cb = res["cpu_baseline"]
    assert cb is not None and cb["value"] > 0 and cb["cores"] == 2 and cb["kind"] == "port"


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """dump_outputs on host tensors: small columns are written whole, large
    ones as the same seeded rows (first and last symbol included) in every
    call, float64, under the 64 MB limit of a dump."""
    import numpy as np
    import torch

    sys.path.insert(0, str(ROOT))
    import bench

    small = {k: torch.arange(35, dtype=torch.float64).reshape(5, 7) + i for i, k in enumerate("ab")}
    info = bench.dump_outputs(small, str(tmp_path / "s"), 1, 0)
    assert info["rows"] == 5 and info["candles"] == 7 and info["nonfinite"] == 0
    cut = bench.dump_outputs(small, str(tmp_path / "cut"), 1, 0, first=3)   # candles before `first` are left out
    assert cut["first_candle"] == 3 and np.array_equal(np.load(tmp_path / "cut" / "a.npy"), small["a"].numpy()[:, 3:])
    assert bench.indicator_warmup() == 100   # ma_100, the longest window of the default set
    assert np.array_equal(np.load(tmp_path / "s" / "b.npy"), small["b"].numpy())
    S, T = 120, 4000   # 14 columns = 54 MB: just over the budget, so rows are sampled
    base = torch.arange(S, dtype=torch.float64)[:, None] * 1e5 + torch.arange(T + 8, dtype=torch.float64)[None, :]
    big = {f"c{i}": (base + i * 1e9)[:, :T] for i in range(14)}   # padded row pitch, as enrich_outputs
    one = bench.dump_outputs(big, str(tmp_path / "one"), 1, 0)
    two = bench.dump_outputs(big, str(tmp_path / "two"), 1, 0)
    assert one["bytes"] == two["bytes"] <= 64 * 2**20 and 2 <= one["rows"] < S and one["candles"] == T
    for k, v in big.items():
        a, b = np.load(tmp_path / "one" / f"{k}.npy"), np.load(tmp_path / "two" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == (one["rows"], T) and np.array_equal(a, b)
        rows = ((a[:, 0] - v[0, 0].item()) / 1e5).astype(np.int64)
        assert rows[0] == 0 and rows[-1] == S - 1 and (np.diff(rows) > 0).all()
        assert np.array_equal(a, v.numpy()[rows])


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_outputs(cuda, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` reports the headline
    and none of the --full legs; --dump-outputs writes the 14 columns of the
    last timed step from the end of the warm-up on, all finite and equal bit
    for bit to enrich on the same seeded panel."""
    import numpy as np

    from binquant_amd import engine
    from binquant_amd._lib import ENRICH_COLUMNS
    from binquant_amd.synth import device_panel

    S, T = 96, 1500
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--symbols", str(S), "--candles", str(T),
                "--dump-outputs", str(tmp_path / "d")], {}, 120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["dtype"] == "f64"
    assert res["value"] == pytest.approx(S * T / (res["ms_per_step"] * 1e-3))
    for leg in ("breadth", "shard", "tick", "store", "rows", "live", "cohort", "cpu_baseline"):
        assert leg not in res
    p = device_panel(S, T, device=cuda, seed=1234)
    want = engine.enrich(p["open"], p["high"], p["low"], p["close"], p["volume"])
    assert sorted(f.name for f in (tmp_path / "d").iterdir()) == sorted(f"{k}.npy" for k in ENRICH_COLUMNS)
    for k in ENRICH_COLUMNS:
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == np.float64 and got.shape == (S, T - 100) and np.isfinite(got).all(), k
        assert np.array_equal(got, want[k].cpu().numpy()[:, 100:]), k
    assert res["dumped_outputs"]["nonfinite"] == 0 and res["dumped_outputs"]["first_candle"] == 100
