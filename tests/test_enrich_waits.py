"""The hot enrich kernel's steady-state loop keeps its memory waits counted.

Compiles bq_enrich.hip to gfx950 assembly (no GPU needed) and reads the tile
loop of enrich_kernel<DIV=0, VOUT=1, DEF=1, HOT=1> with tools/enrich_waits.py.
gfx950's vmcnt counts loads and stores alike, in order: a vmcnt(0) in the loop
would wait for the tile's own 28 output stores, a wait between two prefetch
loads would serialise their round trips to HBM.
"""

import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("enrich_waits", os.path.join(ROOT, "tools", "enrich_waits.py"))
enrich_waits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(enrich_waits)

pytestmark = pytest.mark.skipif(enrich_waits.hipcc_path() is None, reason="hipcc not found")

STORES_PER_TILE = 28   # 14 columns x 2 whole-line stores per lane
LOADS_PER_TILE = 13    # 5 fields x 2 pairs + the neighbour candle's high, low, close


@pytest.fixture(scope="module")
def report():
    asm, remarks = enrich_waits.compile_asm()
    return enrich_waits.analyse(asm, remarks)


@pytest.fixture(scope="module")
def hot_loop(report):
    hot = [r for r in report if r["template"] == "DIV=0 VOUT=1 DEF=1 HOT=1"]
    assert len(hot) == 1, [r["template"] for r in report]
    assert hot[0]["tile_loop"] is not None, "no loop with both barriers and the non-temporal stores"
    print(enrich_waits.render(hot))
    return hot[0]["tile_loop"]


def test_every_instantiation_has_a_tile_loop(report):
    assert len(report) == 9
    assert all(r["tile_loop"] is not None for r in report)


def test_steady_loop_is_the_whole_tile(hot_loop):
    assert hot_loop["barriers"] == 2
    assert hot_loop["global_loads"] == LOADS_PER_TILE
    assert hot_loop["global_stores"] == hot_loop["nt_stores"] == STORES_PER_TILE


def test_steady_loop_never_drains(hot_loop):
    assert [w["text"] for w in hot_loop["waits"] if w["vmcnt"] == 0] == []


def test_prefetch_loads_issue_back_to_back(hot_loop):
    assert hot_loop["waits_between_prefetch_loads"] == 0


def test_prefetched_tile_is_guarded_by_a_counted_wait(hot_loop):
    guards = [w for w in hot_loop["waits"] if w["guards_prefetch"]]
    assert guards, "no wait ahead of the first use of the prefetched tile"
    assert all(w["vmcnt"] >= STORES_PER_TILE for w in guards), [w["text"] for w in guards]
