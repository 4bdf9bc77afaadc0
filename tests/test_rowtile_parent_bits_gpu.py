"""The row-tile kernels whose device code moved write the parent commit's bits.

The kernels of bq_pump / bq_burst / bq_panel / bq_enrich / bq_market /
bq_context / bq_fresh and spike_flags_kernel compile to the parent's assembly
with the helpers of csrc/bq_rowtile.h (`make isa-digest`,
profiles/rowtile_isa.txt) and need no run. spike_base_kernel (the one window
walk sp_walk4), zscore_kernel / adx_kernel and beta_btc_stats_kernel (the
shared block max-scan) do not: this test pins bq_spike_base_std,
bq_spike_base, bq_zscore, bq_adx, bq_wilder_rsi and bq_beta_corr_ws to
tests/golden/rowtile_parent_bits.json, one SHA-256 per output array that the
library built from the commit named in the fixture wrote for the cases of
tools/rowtile_parent_bits.py. The digests cover NaN payloads, the sign of a
zero and the row padding of the output buffers. The fixture is written by
that tool from the parent's library, never from the code under test.

The first tests need no GPU: they show on the host inputs that the cases hold
what makes these kernels go wrong.
"""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("rowtile_parent_bits",
                                               os.path.join(ROOT, "tools", "rowtile_parent_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

GOLDEN = os.path.join(ROOT, "tests", "golden", "rowtile_parent_bits.json")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["seed"] == bits.SEED and len(doc["parent_commit"]) == 40
    assert sorted(doc["digests"]) == sorted(bits.case_id(c) for c in bits.CASES)
    return doc["digests"]


def test_spike_rows_cross_the_tile_with_a_run_and_hold_missing_values():
    x = bits.spike_inputs(2100)
    a, n = bits.SPIKE_RUN
    assert a < 1024 < a + n and a + n - 1024 < 32            # the run spans the boundary, inside the halo
    assert (x["c"][1, a:a + n] == x["c"][1, a]).all() and (x["v"][1, a:a + n] == 0.0).all()
    assert (x["v"][2, a:a + n] < 0.0).all() and (x["v"][2, :a] > 0.0).all()
    assert np.isnan(x["c"][1]).sum() == 1 and np.isposinf(x["c"][1]).sum() == 1
    assert not np.isnan(x["close_ffill"][1]).any() and np.isfinite(x["c"][0]).all()
    assert {(12, 3), (3, 1), (30, 3)} < set(bits.SPIKE_WINDOWS)   # compiled, shorter than a lane, the whole halo
    lds = {T + pad for k, T, pad in bits.CASES if k == "spike_base_std"}
    assert any(ld % 2 for ld in lds) and any(ld % 4 == 2 for ld in lds) and any(ld % 4 == 0 for ld in lds)


def test_signal_and_beta_rows_cross_the_tile_with_a_run():
    x = bits.signal_inputs(4200)
    a, n = bits.SIG_RUN
    assert a < 2048 < a + n
    assert all((x[k][1, a:a + n] == x["close"][1, a]).all() for k in ("high", "low", "close"))
    assert np.isnan(x["close"][2]).sum() == 1 and np.isposinf(x["close"][2]).sum() == 1
    b = bits.beta_inputs(2100)["btc"]
    a, n = bits.BETA_RUN
    assert a < 1024 < a + n and (b[a:a + n] == b[a]).all() and not np.isnan(b).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", bits.CASES, ids=bits.case_id)
def test_entry_point_writes_the_parents_bits(cuda, case):
    got, want = bits.digests(bits.run_case(case, cuda)), golden()[bits.case_id(case)]
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{bits.case_id(case)}: {bad} differ from the parent's bits"
