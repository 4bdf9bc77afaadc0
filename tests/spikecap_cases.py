"""Shared inputs of tests/test_spikecap_ref.py and test_spikecap_gpu.py: the
capped fixture tests/golden/spikecap.npz with its regenerated panel, the
restatement's results on it (computed once, shared) and the synthetic panels
of the kernels' edges with their oracle."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import spikecap_panel_gen as pg           # noqa: E402
import spikecap_ref as cref               # noqa: E402
import spikeframes_ref as ref             # noqa: E402
from spikeframes_cases import (OHLCV, assert_bools_equal, assert_fill, in_frame, same_bits,   # noqa: E402,F401
                               synth_panel)

THRESHOLDS = ("volume_cluster_min_ratio", "price_break_base_threshold")
RTOL = 1e-9   # SURVEY §8c's bar for fp64 against pandas


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "spikecap.npz")
    return {k: z[k] for k in z.files}


def recorded(cap: int) -> dict[str, np.ndarray]:
    """The fixture's cells of one cap under latest_signal()'s names."""
    fx, pre = fixture(), f"c{cap}_"
    return {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.frames_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "spikecap_panel_gen drifted from the recorded inputs"
    return p


@functools.lru_cache(maxsize=8)
def ref_fixture(cap, fast: bool = False, shortcut: bool = False):
    """The restatement on the fixture panel (cap None: the expanding frames), and the zone walks it took."""
    p, zone = panel(), []
    if cap is None:
        return ref.frames(p["open"], p["close"], p["volume"], first_t=p["first_t"], lens=p["lens"]), zone
    kw = dict(fast=True, shortcut=shortcut, zone_walks=zone) if fast else {}
    return cref.frames(p["open"], p["close"], p["volume"], cap, first_t=p["first_t"], lens=p["lens"], **kw), zone


def ties(p, cap, params=None, first_t=None, lens=None) -> int:
    """Near-ties (1e-9 relative, not equal) among every capped frame's comparisons on a panel."""
    S, T = p["close"].shape
    total = 0
    for s in range(S):
        a = 0 if first_t is None else int(first_t[s])
        b = T if lens is None else int(lens[s])
        if b > a:
            total += cref.near_ties(p["open"][s, a:b], p["close"][s, a:b], p["volume"][s, a:b], cap, params)
    return total


def oracle(p, cap, params=None, **kw) -> dict[str, np.ndarray]:
    """The slow restatement on a panel, after asserting that none of its comparisons is a near-tie."""
    rows = {k: kw[k] for k in ("first_t", "lens") if kw.get(k) is not None}
    assert ties(p, cap, params, **rows) == 0, "a near-tie in the case's inputs: pick another seed"
    return cref.frames(p["open"], p["close"], p["volume"], cap, params, **kw)


def assert_thresholds_close(got, want, mask, what):
    for k in THRESHOLDS:
        g, w = got[k][mask], want[k][mask]
        err = np.abs(g - w) / np.abs(w)
        assert np.isfinite(g).all() and (err <= RTOL).all(), f"{what}: {k} off by {np.nanmax(err):.3g} relative"


def assert_matches(got, want, mask, what):
    assert_bools_equal(got, want, mask, what)
    assert_thresholds_close(got, want, mask, what)
    if "close_open_ratio" in want and "close_open_ratio" in got:
        assert same_bits(got["close_open_ratio"][mask], want["close_open_ratio"][mask]).all(), what
    assert_fill(got, mask, what)


def tiled(p, S: int) -> dict[str, np.ndarray]:
    """Row s of the result is row s % len(p) of p: more rows than a workgroup holds, one oracle."""
    idx = np.arange(S) % len(next(iter(p.values())))
    return {k: np.ascontiguousarray(v[idx]) for k, v in p.items()}


def gap_at_frame_start(T: int = 200, cap: int = 64, seed: int = 414) -> dict[str, np.ndarray]:
    """Three rows whose close (and volume) is missing exactly on the first row of chosen capped frames, the
    close just before it valid: rows 30 (alone), 60 .. 65 (a run: the frame that starts inside it has its
    first price change more than 4 rows in, so its newest row's quantile window is cut) and 100, 101."""
    p = synth_panel(3, T, seed, kind="mixed")   # a quiet, a dense and a noisy row (its price floor is raised)
    for k in ("close", "volume", "quote_asset_volume"):
        p[k] = p[k].copy()
        p[k][:, [30, 60, 61, 62, 63, 64, 65, 100, 101]] = np.nan
    return p
