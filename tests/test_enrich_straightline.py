"""The hot enrich kernel's steady-state loop is straight-line code.

Compiles bq_enrich.hip to gfx950 assembly (no GPU needed) and reads the tile
loop of enrich_kernel<DIV=0, VOUT=1, DEF=1, HOT=1> with tools/enrich_waits.py.
An exec-mask region is a scheduling boundary: an LDS read inside one can be
neither hoisted nor batched with its neighbours, and its round trip is waited
for (lgkmcnt(0)) inside the region. The loop keeps one such region — the halo
copy, which only the last 32 lanes of the workgroup take — no exec-mask loop,
and stays inside the register budget of 3 waves per SIMD without touching
scratch memory.

PARENT_* are the tool's counts for the loop as it stood before the per-lane
branches were replaced by selects; LGKM0_WAITS and INSTRUCTIONS those of the
loop as committed with this test.
"""

import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("enrich_waits", os.path.join(ROOT, "tools", "enrich_waits.py"))
enrich_waits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(enrich_waits)

pytestmark = pytest.mark.skipif(enrich_waits.hipcc_path() is None, reason="hipcc not found")

LOADS_PER_TILE = 13
PARENT_LGKM0_WAITS = 71
PARENT_INSTRUCTIONS = 2720
LGKM0_WAITS = 30
INSTRUCTIONS = 2533


@pytest.fixture(scope="module")
def report():
    asm, remarks = enrich_waits.compile_asm()
    return enrich_waits.analyse(asm, remarks)


@pytest.fixture(scope="module")
def hot(report):
    recs = [r for r in report if r["template"] == "DIV=0 VOUT=1 DEF=1 HOT=1"]
    assert len(recs) == 1, [r["template"] for r in report]
    assert recs[0]["tile_loop"] is not None
    print(enrich_waits.render(recs))
    return recs[0]


def test_every_instantiation_still_has_its_tile_loop(report):
    assert len(report) == 9
    assert all(r["tile_loop"] is not None for r in report), [r["template"] for r in report if r["tile_loop"] is None]


def test_register_and_lds_budget(hot):
    res = hot["resources"]
    assert res["VGPRs"] <= 168
    assert res["Occupancy"] == 3
    assert res["LDS Size"] <= 52032


def test_loop_touches_no_scratch_and_never_drains(hot):
    loop = hot["tile_loop"]
    assert loop["scratch_ops"] == 0
    assert [w["text"] for w in loop["waits"] if w["vmcnt"] == 0] == []
    assert loop["global_loads"] == LOADS_PER_TILE and loop["waits_between_prefetch_loads"] == 0


def test_halo_copy_is_the_only_masked_region_reading_lds(hot):
    cf = hot["tile_loop"]["control_flow"]
    assert cf["exec_regions_with_lds_read"] == 1, cf


def test_no_exec_mask_loop(hot):
    assert hot["tile_loop"]["control_flow"]["exec_loops"] == 0


def test_fewer_lds_drains_and_instructions_than_the_parent(hot):
    loop = hot["tile_loop"]
    cf = loop["control_flow"]
    assert cf["lgkmcnt0_waits"] <= LGKM0_WAITS < PARENT_LGKM0_WAITS, cf
    assert loop["instructions"] <= INSTRUCTIONS < PARENT_INSTRUCTIONS, loop["instructions"]
    assert sum(cf["classes"].values()) == loop["instructions"]
