"""The wave-per-row replay entry points write the parent commit's bits.

bq_retest, bq_spikefade, bq_pricetracker, bq_meanrev and bq_rangefade took
their scaffolding from csrc/bq_replay.h and no longer compile to the parent's
assembly (`make isa-digest`, profiles/replay_isa.txt), so this test pins
bq_retest_replay, bq_spike_fade_replay, bq_price_tracker_replay,
bq_mean_reversion_replay and bq_range_fade_replay to
tests/golden/replay_parent_bits.json: one SHA-256 per output array and per
state array after the call that the library built from the commit named in
the fixture wrote for the cases of tools/replay_parent_bits.py. The digests
cover NaN payloads and the sign of a zero. The fixture is written by that tool
from the parent's library, never from the code under test.

The first tests need no GPU: they show on the host inputs that the cases hold
what the hoisted paths need.
"""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("replay_parent_bits",
                                               os.path.join(ROOT, "tools", "replay_parent_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

GOLDEN = os.path.join(ROOT, "tests", "golden", "replay_parent_bits.json")
WAVE = 64


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["seed"] == bits.SEED and len(doc["parent_commit"]) == 40
    assert sorted(doc["digests"]) == sorted(bits.case_id(c) for c in bits.CASES)
    return doc["digests"]


def test_rows_reach_the_prelude_and_the_warm_up():
    assert bits.S == 6 and set(bits.SHAPES) == {1, 63, 64, 65, 130, 200}   # two workgroups, the second half empty
    for T in (130, 200):
        r = bits.rows(T)
        first, frm, lens = r["first_t"], r["from_t"], r["lens"]
        assert first[1] % WAVE != 0 and first[4] % WAVE != 0                     # first_t mid-step
        assert frm[2] // WAVE - first[2] // WAVE == 2 and frm[2] < lens[2]        # two warm-up steps, then a replay
        assert lens[3] < T and frm[5] >= lens[5]                                  # a short row, a row with no replay
    assert all(sorted({c[1] for c in bits.CASES if c[0] == e and c[2] == "base"}) == sorted(bits.SHAPES)
               for e in bits.VARIANTS)


@pytest.mark.parametrize("entry", ["price_tracker", "mean_reversion"])
def test_in_pass_series_meet_the_serial_switch_and_the_flat_stretch(entry):
    for T in (130, 200):
        p, r = bits.inputs(entry, T), bits.rows(T)
        c, first, lens = p["close"], r["first_t"], r["lens"]
        s, t = bits.NAN_SECOND_STEP
        assert np.isnan(c[s, t]) and first[s] // WAVE + 1 == t // WAVE and t < lens[s]   # the frame's second step
        assert np.isfinite(c[s, first[s]:t]).all()                                      # a seeded carry
        assert np.isnan(c[4, first[4]])                                                  # missing at first_t itself
        assert np.isposinf(c[bits.INF_AT]) and bits.INF_AT[1] >= first[bits.INF_AT[0]]
        s, a, n = bits.FLAT
        assert (c[s, a:a + n] == c[s, a]).all() and a >= first[s] and a + n <= lens[s]


def test_variants_cover_the_argument_layer():
    from binquant_amd import _lib

    v = bits.VARIANTS
    assert {"tail1", "cd0", "cd3", "nohlv", "trend"} <= set(v["price_tracker"])
    assert all({"ctx1", "bare", "pitch"} <= set(v[e]) for e in ("price_tracker", "mean_reversion", "range_fade"))
    assert all({"wmax", "feat"} <= set(v[e]) for e in ("mean_reversion", "range_fade"))
    assert all({"bare", "pitch"} <= set(v[e]) for e in ("retest", "spike_fade")) and "shared" in v["spike_fade"]
    assert _lib.MR_MAX_WINDOW > 20 and _lib.RF_MAX_ADX_WINDOW > 14 and _lib.RF_MAX_ZSCORE_WINDOW > 20
    p = bits.inputs("range_fade", bits.TV)
    assert np.isnan(p["close"][1, 70]) and np.isnan(p["high"][4, 7])


@pytest.mark.gpu
@pytest.mark.parametrize("case", bits.CASES, ids=bits.case_id)
def test_entry_point_writes_the_parents_bits(cuda, case):
    got, want = bits.digests(bits.run_case(case, cuda)), golden()[bits.case_id(case)]
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{bits.case_id(case)}: {bad} differ from the parent's bits"
