"""The hot enrich kernel's line-ordered prefetch and in-wave neighbour candle.

Behind tile 0 the hot kernel loads each field in line order (lane L the pairs
at line_offset<4>(L) and 128 candles on, one contiguous KiB per instruction),
exchanges the pairs back where the tile is consumed, and takes the neighbour
candle of lanes 1-63 from the lane before. The partial tail is selected pair
by pair on the loading lane, ahead of the exchange. The generic kernels (a
call that omits one column) load every tile in lane order with range-checked
loads, so the two must agree in every bit of every column, NaN payloads
included.

Lengths: one whole tile plus a tail that ends inside the first 128-candle
half of a wave's slice, on that half's edge, on a wave's edge (256, 512, 768),
at odd lengths, and one candle short of a whole tile; two longer lengths reach
the tail from the steady loop. Layouts: contiguous rows (odd T then leaves the
rows 8-byte aligned: the generic kernels on both sides) and rows on an even
pitch (16-byte aligned at odd T too: the hot kernel's tail ends on a moved
pair) inside SENTINEL-filled buffers, where nothing past T may be written.
"""

import functools

import numpy as np
import pytest
import torch

from binquant_amd import engine
from binquant_amd._lib import ENRICH_COLUMNS, INPUT_FIELDS
from binquant_amd.synth import numpy_panel

pytestmark = pytest.mark.gpu

S = 3
TAILS = [2, 3, 126, 127, 128, 129, 130, 131, 254, 255, 256, 257, 258, 383, 385, 511, 513, 767, 769, 1022, 1023]
LENGTHS = [1024 + d for d in TAILS] + [2048 + 129, 3072 + 255]
LAYOUTS = ["contiguous", "pitched"]
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def host_panel():
    """one walk of the longest length; every case reads a prefix of it"""
    panel = numpy_panel(S, max(LENGTHS), seed0=4242)
    for v in panel.values():
        v.setflags(write=False)
    return panel


def pitched(x, pitch):
    """x as a [S, T] view of a fresh SENTINEL-filled buffer with the given row pitch"""
    s, t = x.shape
    buf = torch.full((s * pitch,), SENTINEL, dtype=torch.float64, device=x.device)
    view = buf.view(s, pitch)[:, :t]
    view.copy_(x)
    return buf, view


def pitch_of(T, layout):
    return T if layout == "contiguous" else T + 192 + (T & 1)


def device_inputs(panel, T, dev, layout):
    ins = [torch.from_numpy(np.array(panel[f][:, :T])).to(dev) for f in INPUT_FIELDS]
    return [pitched(x, pitch_of(T, layout))[1] for x in ins]


def run(ins, T, layout, columns=ENRICH_COLUMNS):
    """enrich into fresh outputs of the layout; everything past T must stay SENTINEL"""
    dev = ins[0].device
    blank = torch.empty((S, T), dtype=torch.float64, device=dev)
    outs = {}
    for c in columns:
        buf, view = pitched(blank, pitch_of(T, layout))
        buf.fill_(SENTINEL)
        outs[c] = (buf, view)
    got = engine.enrich(*ins, columns=columns, out={c: v for c, (_, v) in outs.items()})
    torch.cuda.synchronize()
    for c, (buf, view) in outs.items():
        pad = buf.view(S, view.stride(0))[:, T:]
        assert bool((pad == SENTINEL).all()), f"{c}: a store landed past T ({layout}, T={T})"
    return {c: got[c].contiguous() for c in columns}


def run_generic(ins, T, layout):
    """all 14 columns through the generic kernels: two calls, each omitting one column"""
    a = run(ins, T, layout, columns=ENRICH_COLUMNS[:-1])
    b = run(ins, T, layout, columns=ENRICH_COLUMNS[1:])
    return {**b, **a}


def assert_same(got, want, what):
    g, w = got.view(torch.int64), want.view(torch.int64)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        r, t = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at row {r} candle {t}: "
                             f"{float(got[r, t])!r} != {float(want[r, t])!r}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T", LENGTHS)
def test_line_ordered_tail_equals_generic_path(cuda, T, layout):
    ins = device_inputs(host_panel(), T, cuda, layout)
    hot = run(ins, T, layout)
    gen = run_generic(ins, T, layout)
    for c in ENRICH_COLUMNS:
        assert_same(hot[c], gen[c], f"{c}, T={T}, {layout}: all 14 columns vs a call omitting one")


def test_flagged_row_with_nan_first_and_last_candle(cuda):
    """row 1 has no first and no last candle: the walk flags it from tile 0
    and from the tail's moved pair, and the rewrite sees the row it saw before"""
    T, layout = 2048 + 129, "pitched"
    clean = {k: v[:, :T] for k, v in host_panel().items()}
    dirty = {k: v.copy() for k, v in clean.items()}
    for f in INPUT_FIELDS:
        dirty[f][1, 0] = np.nan
        dirty[f][1, T - 1] = np.nan
    ins = device_inputs(dirty, T, cuda, layout)
    hot = run(ins, T, layout)
    gen = run_generic(ins, T, layout)
    base = run(device_inputs(clean, T, cuda, layout), T, layout)
    for c in ENRICH_COLUMNS:
        assert_same(hot[c], gen[c], f"{c}: a row with NaN first and last candles")
        assert_same(hot[c][[0, 2]], base[c][[0, 2]], f"{c}: clean rows beside the rewritten one")
    assert bool(torch.isnan(hot["ma_7"][1, :7]).all()) and not bool(torch.isnan(hot["ma_7"][1, 7]))
    assert bool(torch.isnan(hot["ma_7"][1, T - 1])) and not bool(torch.isnan(hot["ma_7"][1, T - 2]))
    assert bool(torch.isnan(hot["ema20"][1, 0])) and not bool(torch.isnan(hot["ema20"][1, T - 1]))
