"""tests/golden/strategy_gaps.npz (+ strategy_gaps_fsf.npz): loading, the
regenerated inputs and the comparison rules shared by
tests/test_strategy_gaps.py and tests/test_strategy_gaps_gpu.py.

The fixture is written by tests/golden/make_golden_strategy_gaps.py from the
REAL reference on the rows of tests/golden/strategy_gaps_panel_gen.py."""

from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np

G = Path(__file__).resolve().parent / "golden"

_spec = importlib.util.spec_from_file_location("strategy_gaps_panel_gen", G / "strategy_gaps_panel_gen.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

TAGS = {"short": (gen.SHORT_CASES, gen.T_SHORT, 0, 0), "long": (gen.LONG_CASES, gen.T_LONG, gen.LONG_FROM,
                                                                len(gen.SHORT_CASES))}   # cases, T, first recorded, row0
CASES = [(tag, i, case) for tag, (cases, _, _, _) in TAGS.items() for i, case in enumerate(cases)]

_cache: dict = {}


def load() -> dict[str, np.ndarray]:
    """Both files as one mapping (read once)."""
    if "z" not in _cache:
        z = {}
        for name in ("strategy_gaps.npz", "strategy_gaps_fsf.npz"):
            with np.load(G / name) as f:
                z.update({k: f[k] for k in f.files})
        _cache["z"] = z
    return _cache["z"]


def panels() -> dict[str, dict[str, np.ndarray]]:
    """The regenerated inputs {tag: {field: [S, T]}}; asserts the stored digest
    and that the stored inputs are the regenerated ones."""
    if "p" not in _cache:
        z = load()
        P = {"short": gen.short_panel(), "long": gen.long_panel()}
        assert gen.digest(P["short"], P["long"]) == str(z["digest"]), "panel generator drifted from the recorded inputs"
        for tag, p in P.items():
            for f in gen.FIELDS:
                np.testing.assert_array_equal(p[f], z[f"{tag}__{f}"], err_msg=f"{tag}.{f}")
        _cache["p"] = P
    return _cache["p"]


def bench_aligned(tag: str) -> np.ndarray:
    """The benchmark left-merged onto the panel's grid: NaN where it has no candle."""
    z = load()
    keep, close = gen.bench_series(TAGS[tag][1])
    np.testing.assert_array_equal(keep, z[f"{tag}__bench_keep"])
    np.testing.assert_array_equal(close, z[f"{tag}__bench_close"])
    return np.where(keep, close, np.nan)


def columns(prefix: str) -> list[str]:
    z = load()
    return sorted(k.split("__", 2)[2] for k in z if k.startswith(f"short__{prefix}__"))


def row_scale(w: np.ndarray) -> float:
    """The row's largest finite recorded magnitude of a column (1.0 if none)."""
    w = np.asarray(w, dtype=np.float64)
    fin = np.abs(w[np.isfinite(w)])
    sc = float(fin.max()) if fin.size else 1.0
    return sc if sc > 0 else 1.0


def first_violation(g, w, rtol: float = 1e-9, atol_rel: float = 1e-11):
    """(index, error in units of the bar) of the first cell of a row where
    tests.util.assert_close(g, w, rtol, scale=row_scale(w)) would fail, with
    the worst error of the row; None if it passes. Flags: any difference."""
    g, w = np.asarray(g), np.asarray(w)
    if g.dtype == bool or w.dtype == np.uint8:
        bad = g.astype(np.int64) != w.astype(np.int64)
        return (int(np.argmax(bad)), float(bad.sum())) if bad.any() else None
    g, w = g.astype(np.float64), w.astype(np.float64)
    lim = rtol * np.abs(w) + atol_rel * row_scale(w)
    with np.errstate(all="ignore"):
        err = np.abs(g - w) / lim
    same = (np.isnan(g) & np.isnan(w)) | (np.isinf(w) & (g == w))
    bad = ~same & ~(err <= 1.0)
    if not bad.any():
        return None
    worst = np.where(bad, np.nan_to_num(err, nan=np.inf, posinf=np.inf), 0.0).max()
    return int(np.argmax(bad)), float(worst)
