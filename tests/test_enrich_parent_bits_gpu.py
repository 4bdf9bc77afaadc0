"""bq_enrich's output bits are those of the parent commit's library.

tests/test_enrich_tiles_gpu.py compares the hot kernel with the generic ones;
once the tile body they share changes, both can move together. This test pins
both to tests/golden/enrich_parent_bits.json: a SHA-256 per (column, row,
256-candle block) of the outputs that the library built from the commit named
in the fixture wrote for the panel of tools/enrich_parent_bits.py (S = 6,
T = 2832 and 1025; rows 1..5 carry constant closes, strictly rising / falling
runs, zero volume, identical OHLC bars and closes alternating between adjacent
doubles, each placed inside a lane, on a lane, wave and tile boundary and
inside the warm-up). The digests cover NaN payloads and the sign of a zero.
The fixture is written by that tool from the parent's library, never from the
code under test.

The first test needs no GPU: the pandas oracle on the same panel shows that
every case the kernel's selects decide does occur past the warm-up, so the
panel can fail for the right reasons.
"""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("enrich_parent_bits",
                                               os.path.join(ROOT, "tools", "enrich_parent_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

GOLDEN = os.path.join(ROOT, "tests", "golden", "enrich_parent_bits.json")
WARM = 100   # the longest window: every output is defined from candle 99 on


@functools.lru_cache(maxsize=None)
def host_panel(T):
    panel = bits.build_panel(T)
    for v in panel.values():
        v.setflags(write=False)
    return panel


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["seed"] == bits.SEED and doc["block"] == bits.BLOCK and doc["rows"] == bits.S
    assert len(doc["parent_commit"]) == 40
    return doc["digests"]


@pytest.mark.parametrize("T", bits.LENGTHS)
def test_panel_holds_every_case_past_the_warm_up(T):
    import pandas as pd

    from oracle import indicators_ref as ref

    p = host_panel(T)
    seen = {k: 0 for k in ("rsi 100", "rsi 0", "rsi nan", "mfi 100", "mfi 0", "mfi nan", "bb_upper == bb_mid",
                           "atr 0", "twap constant")}
    for s in range(bits.S):
        df = ref.indicators_enrichment(pd.DataFrame({f: np.array(p[f][s]) for f in p}))
        col = {k: df[k].to_numpy()[WARM:] for k in ("rsi", "mfi", "bb_upper", "bb_mid", "ATR", "twap", "close")}
        assert not np.isnan(col["bb_mid"]).any() and not np.isnan(col["ATR"]).any()
        one = {"rsi 100": col["rsi"] == 100.0, "rsi 0": col["rsi"] == 0.0, "rsi nan": np.isnan(col["rsi"]),
               "mfi 100": col["mfi"] == 100.0, "mfi 0": col["mfi"] == 0.0, "mfi nan": np.isnan(col["mfi"]),
               "bb_upper == bb_mid": col["bb_upper"] == col["bb_mid"], "atr 0": col["ATR"] == 0.0,
               "twap constant": (col["twap"][1:] == col["twap"][:-1]) & (col["close"][1:] == col["close"][:-1])}
        if s == 0:
            continue   # the plain walk; its own constant runs do not count
        for k, m in one.items():
            seen[k] += int(m.sum())
    assert all(n > 0 for n in seen.values()), seen


def _check(T, got, what):
    bad = bits.mismatches(bits.digests(got), golden()[str(T)])
    assert not bad, f"T={T}, {what}: {len(bad)} blocks differ from the parent's bits: " + "; ".join(bad[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("T", bits.LENGTHS)
def test_hot_kernel_writes_the_parents_bits(cuda, T):
    _check(T, bits.run_hot(bits.device_inputs(host_panel(T), cuda)), "all 14 columns in one call")


@pytest.mark.gpu
@pytest.mark.parametrize("T", bits.LENGTHS)
def test_generic_kernels_write_the_parents_bits(cuda, T):
    _check(T, bits.run_generic(bits.device_inputs(host_panel(T), cuda)), "two calls omitting one column each")
