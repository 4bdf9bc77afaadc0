"""The market-context entry points write the parent commit's bits.

bq_breadth_partial and bq_breadth_partial_fresh share one templated kernel
pair, and the feature kernels share their host setup; the tests that compare
the members of this family with each other move together when the shared code
changes. This test pins each entry point to
tests/golden/context_parent_bits.json: one SHA-256 per output array that the
library built from the commit named in the fixture wrote for the cases of
tools/context_parent_bits.py (both breadth kernels dense and fresh, both
feature kernels, the ring / lagged-chain context build, the compaction). The
digests cover NaN payloads and the sign of a zero. The fixture is written by
that tool from the parent's library, never from the code under test.

The first two tests need no GPU: they show on the host panels that the cases
can fail for the right reasons.
"""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("context_parent_bits",
                                               os.path.join(ROOT, "tools", "context_parent_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

GOLDEN = os.path.join(ROOT, "tests", "golden", "context_parent_bits.json")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["seed"] == bits.SEED and len(doc["parent_commit"]) == 40
    assert sorted(doc["digests"]) == sorted(bits.case_id(c) for c in bits.CASES)
    return doc["digests"]


@pytest.mark.parametrize("case", [c for c in bits.CASES if c[0] == "breadth"], ids=bits.case_id)
def test_dense_breadth_inputs_hold_nan_returns(case):
    from oracle import market_ref

    _, S, T, M = case
    h, l, c = bits.host_inputs(case)
    # candle 0 of every row has a one-candle history: no features, a NaN return
    assert all(market_ref.panel_features_at(h[s], l[s], c[s], 0, M) is None for s in range(S))
    if T > 1:
        assert market_ref.panel_features_at(h[0], l[0], c[0], T - 1, M) is not None


@pytest.mark.parametrize("case", [c for c in bits.CASES if c[0] in ("breadth_fresh", "compact")], ids=bits.case_id)
def test_sparse_panels_hold_an_empty_and_a_full_timestamp(case):
    _, S, T, _ = case
    *_, present = bits.sparse_panel(S, T)
    first = np.where(present.any(axis=1), present.argmax(axis=1), T)
    listed = first[:, None] <= np.arange(T)[None, :]
    n_present, n_listed = present.sum(axis=0), listed.sum(axis=0)
    assert n_present[bits.T_EMPTY] == 0 and n_listed[bits.T_EMPTY] > 0
    assert n_present[bits.T_FULL] == n_listed[bits.T_FULL] > 1
    assert (first == T).sum() == 1 and ((first > 0) & (first < T)).any()   # one never present, a late listing
    assert (n_present < n_listed).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", bits.CASES, ids=bits.case_id)
def test_entry_point_writes_the_parents_bits(cuda, case):
    got, want = bits.digests(bits.run_case(case, cuda)), golden()[bits.case_id(case)]
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{bits.case_id(case)}: {bad} differ from the parent's bits"
