#!/usr/bin/env python3
"""Pin the output bits of the row-tile kernels whose device code moved when
their helpers went to csrc/bq_rowtile.h: the cases and their digests.

`make isa-digest` shows which kernel files compile to the parent commit's
assembly; the kernels that do not (spike_base_kernel: the shared window walk
sp_walk4; zscore_kernel / adx_kernel and beta_btc_stats_kernel: the shared
block max-scan, which reads the tile carry after its barrier) are compared
here, bit for bit, with the library of the parent commit.
tests/test_rowtile_parent_bits_gpu.py runs the cases; this file holds what the
test and the fixture writer share and, run as a script, writes the fixture:

  BQ_LIB_PATH=<library built from the parent commit> \\
      python tools/rowtile_parent_bits.py --commit <parent id> --out tests/golden/rowtile_parent_bits.json

The fixture is written from the parent's library only: BQ_LIB_PATH must be set
and must not name this tree's own library. It holds one SHA-256 per output
array, so a NaN's payload and the sign of a zero count. Output buffers are
hashed whole, their row padding (ld > T) included: a store past T shows.

The cases, S = 3 rows each:

  spike_base_std / spike_base   (tile 1024, halo 32, 4 candles per lane)
      T = 1 / 3 / 1023 / 1024 / 1025 / 2100 at ld = T, and T = 2100 at
      ld = T + 1 (scalar doubles, scalar flag bytes) and ld = T + 2 (16-byte
      doubles, scalar flag bytes; ld = T = 2100 / 1024 take the dword flag
      store). Each with (base_window, streak_length) = (12, 3) the compiled
      instantiation, (7, 2) the run-time one, (3, 1) the per-candle branch of
      windows shorter than a lane, (30, 3) a window over the whole usable halo.
      Rows: a plain walk; a row with a NaN, a +inf and 40 equal closes with
      zero volume (missing-in-window and the same-value rule; at T = 2100 the
      run spans the tile boundary at 1024); a row whose volume is negative for
      those 40 candles (the mean's sign rule).
  zscore / adx / wilder_rsi     (tile 2048, halo 128, 8 candles per lane)
      T = 1 / 2047 / 2048 / 2049 / 4200, and T = 2048 read through an odd row
      stride (the scalar load path); the compiled window (20 / 14 / 14) and
      that window plus one. Rows: a plain walk; a constant run over the tile
      boundary at 2048; a row with a NaN and a +inf.
  beta_corr (bq_beta_corr_ws)   T = 1 / 1023 / 1025 / 2100, windows 50 and 20;
      the benchmark row holds a run of equal closes over the pre-pass's tile
      boundary at 1024. Every close is finite: rows with missing or zero
      closes are judged against the reference, not the parent
      (tests/test_beta_gaps_gpu.py).
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261019
S = 3
NAN = float("nan")
SPIKE_WINDOWS = ((12, 3), (7, 2), (3, 1), (30, 3))
SPIKE_RUN = (1000, 40)   # start, length of the equal-close / signed-volume run
SIG_WINDOWS = {"zscore": (20, 21), "adx": (14, 15), "wilder_rsi": (14, 15)}
SIG_RUN = (2040, 20)
BETA_WINDOWS = (50, 20)
BETA_RUN = (1010, 30)

# (kind, T, pad): pad = ld - T of the spike buffers, or of the signal inputs' row stride
CASES = (
    [(k, T, 0) for k in ("spike_base_std", "spike_base") for T in (1, 3, 1023, 1024, 1025, 2100)]
    + [(k, 2100, pad) for k in ("spike_base_std", "spike_base") for pad in (1, 2)]
    + [(k, T, 0) for k in SIG_WINDOWS for T in (1, 2047, 2048, 2049, 4200)]
    + [(k, 2048, 1) for k in SIG_WINDOWS]
    + [("beta_corr", T, 0) for T in (1, 1023, 1025, 2100)]
)


def case_id(case) -> str:
    kind, T, pad = case
    return f"{kind}/{T}+{pad}"


def _walk(g, T: int):
    """open, high, low, close, volume [S, T] of a random walk"""
    c = 50.0 * np.exp(np.cumsum(g.normal(0.0, 0.004, (S, T)), axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    h = np.maximum(o, c) * (1.0 + g.uniform(0.0, 0.003, (S, T)))
    l = np.minimum(o, c) * (1.0 - g.uniform(0.0, 0.003, (S, T)))
    return o, h, l, c, g.lognormal(3.0, 1.0, (S, T))


def _run(T: int, start: int, length: int) -> slice:
    a = max(0, min(T - 1, start))
    return slice(a, min(T, a + length))


def _ffill(x: np.ndarray) -> np.ndarray:
    idx = np.where(np.isnan(x), 0, np.arange(x.shape[1])[None, :])
    np.maximum.accumulate(idx, axis=1, out=idx)
    return np.take_along_axis(x, idx, axis=1)


def spike_inputs(T: int) -> dict[str, np.ndarray]:
    g = np.random.default_rng(SEED + T)
    o, h, l, c, v = _walk(g, T)
    r = _run(T, *SPIKE_RUN)
    for x in (o, h, l, c):
        x[1, r] = c[1, r.start]
    v[1, r] = 0.0
    v[2, r] = -v[2, r]
    if T > 8:
        c[1, T // 2] = NAN
        c[1, T // 4] = np.inf
    ins = {"o": o, "h": h, "l": l, "c": c, "v": v, "qv": v * c, "close_ffill": _ffill(c)}
    # bq_spike_base reads its five std columns: any positive values, NaN while a window fills
    for n in ("price_std", "volume_std", "std8", "std20", "body_pct_std"):
        sd = g.uniform(0.01, 2.0, (S, T))
        sd[:, :7] = NAN
        ins[n] = sd
    return ins


def signal_inputs(T: int) -> dict[str, np.ndarray]:
    g = np.random.default_rng(SEED + 3 * T + 1)
    _, h, l, c, _ = _walk(g, T)
    r = _run(T, *SIG_RUN)
    for x in (h, l, c):
        x[1, r] = c[1, r.start]
    if T > 8:
        c[2, T // 2] = NAN
        c[2, T // 4] = np.inf
    return {"high": h, "low": l, "close": c}


def beta_inputs(T: int) -> dict[str, np.ndarray]:
    g = np.random.default_rng(SEED + 5 * T + 2)
    c = _walk(g, T)[3]
    btc = 60000.0 * np.exp(np.cumsum(g.normal(0.0, 0.001, T)))
    r = _run(T, *BETA_RUN)
    btc[r] = btc[r.start]
    return {"close": c, "btc": btc}


def _padded(x: np.ndarray, ld: int, dev):
    """x [S, T] in the first T columns of a [S, ld] device buffer"""
    import torch

    buf = torch.full((x.shape[0], ld), -7.0, dtype=torch.float64, device=dev)
    buf[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return buf


def _run_spike(kind: str, T: int, pad: int, dev) -> dict:
    import torch

    from binquant_amd import _lib, engine

    ld = T + pad
    ins = spike_inputs(T)
    names = ("o", "h", "l", "c", "v", "qv", "close_ffill")
    if kind == "spike_base":
        names += ("price_std", "volume_std", "std8", "std20", "body_pct_std")
    bufs = [_padded(ins[n], ld, dev) for n in names]
    lib = _lib.load()
    out = {}
    for w, n in SPIKE_WINDOWS:
        f = {c: torch.full((S, ld), -7.0, dtype=torch.float64, device=dev) for c in engine.SPIKE_BASE_FLOAT}
        b = {c: torch.full((S, ld), 3, dtype=torch.uint8, device=dev) for c in engine.SPIKE_BASE_BOOL}
        sd = {c: torch.full((S, ld), -7.0, dtype=torch.float64, device=dev) for c in engine.SPIKE_STD}
        args = [_lib.ptr_array([t.data_ptr() for t in bufs]), S, T, ld, w, n,
                _lib.ptr_array([t.data_ptr() for t in f.values()]), _lib.ptr_array([t.data_ptr() for t in b.values()])]
        if kind == "spike_base_std":
            args.append(_lib.ptr_array([t.data_ptr() for t in sd.values()]))
        _lib.check(getattr(lib, "bq_" + kind)(*args, ld, engine._stream_handle(None)), "bq_" + kind)
        cols = {**f, **b, **(sd if kind == "spike_base_std" else {})}
        out.update({f"w{w}n{n}/{c}": t for c, t in cols.items()})
    return out


def run_case(case, dev) -> dict[str, np.ndarray]:
    """the case's output arrays, on the host"""
    import torch

    from binquant_amd import engine

    kind, T, pad = case
    if kind.startswith("spike_base"):
        out = _run_spike(kind, T, pad, dev)
    elif kind in SIG_WINDOWS:
        x = {k: _padded(v, T + pad, dev)[:, :T] for k, v in signal_inputs(T).items()}
        assert x["close"].stride(0) == T + pad
        ins = (x["high"], x["low"], x["close"]) if kind == "adx" else (x["close"],)
        out = {f"w{w}": getattr(engine, kind)(*ins, window=w) for w in SIG_WINDOWS[kind]}
    elif kind == "beta_corr":
        x = beta_inputs(T)
        close, btc = (torch.from_numpy(np.ascontiguousarray(x[k])).to(dev) for k in ("close", "btc"))
        out = {f"w{w}/{k}": v for w in BETA_WINDOWS for k, v in engine.beta_corr(close, btc, w).items()}
    else:
        raise ValueError(kind)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def digests(out: dict[str, np.ndarray]) -> dict[str, str]:
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in out.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="id of the commit the library in BQ_LIB_PATH was built from")
    ap.add_argument("--out", required=True, help="fixture to write (tests/golden/rowtile_parent_bits.json)")
    args = ap.parse_args()
    lib = os.environ.get("BQ_LIB_PATH")
    own = os.path.join(ROOT, "binquant_amd", "lib", "libbinquant_amd.so")
    if not lib or os.path.realpath(lib) == os.path.realpath(own):
        print("BQ_LIB_PATH must name a library built from the parent commit, not this tree's own: the fixture "
              "is never written from the code under test", file=sys.stderr)
        return 2
    if len(args.commit) != 40:
        print("--commit: the full 40-character id", file=sys.stderr)
        return 2
    import torch

    from binquant_amd import _lib

    dev = torch.device("cuda:0")
    doc = {"parent_commit": args.commit, "seed": SEED, "library": _lib.load().bq_version().decode(),
           "digests": {case_id(c): digests(run_case(c, dev)) for c in CASES}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {sum(len(d) for d in doc['digests'].values())} digests from {_lib.LIB_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
