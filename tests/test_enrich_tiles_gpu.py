"""The hot enrich kernel against the generic ones, bit for bit.

bq_enrich sends the common call (all 14 columns, 16-byte aligned rows, the
reference's windows, integer EMA spans) to enrich_kernel<.., HOT>, whose tile
chain is peeled: tile 0, a branch-free loop over the whole interior tiles, the
partial tail. A call that omits one column takes a generic instantiation, so
the two must agree in every bit of every column. The lengths cover: below the
halo, one partial tile, the tile boundary and its neighbours, two whole tiles
plus a 784-candle tail (the headline's tail), and three and four whole tiles
(the steady loop runs more than once). Layouts: contiguous rows; outputs as
[:, :T] views of [S, T + 192] buffers; inputs and outputs on an even pitch,
which keeps the rows 16-byte aligned at odd T too (the hot kernel's tail then
ends on an 8-byte aligned pair). The values themselves are pinned against the
pandas oracle by tests/test_enrich_gpu.py.
"""

import functools

import numpy as np
import pytest
import torch

from binquant_amd import engine
from binquant_amd._lib import ENRICH_COLUMNS, INPUT_FIELDS
from binquant_amd.synth import numpy_panel

pytestmark = pytest.mark.gpu

S = 5
LENGTHS = [3, 130, 1023, 1024, 1025, 2048, 2050, 2832, 3088, 4096]
LAYOUTS = ["contiguous", "padded", "pitched"]
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def host_panel(T):
    panel = numpy_panel(S, T, seed0=T)
    for v in panel.values():
        v.setflags(write=False)
    return panel


def pitched(x, pitch, shift=0):
    """x as a [S, T] view of a fresh buffer with the given row pitch, the rest
    of the buffer holding SENTINEL; shift moves the view by whole elements"""
    s, t = x.shape
    buf = torch.full((s * pitch + shift,), SENTINEL, dtype=torch.float64, device=x.device)
    view = buf[shift:shift + s * pitch].view(s, pitch)[:, :t]
    view.copy_(x)
    return buf, view


def device_inputs(panel, dev, layout):
    T = panel["close"].shape[1]
    ins = [torch.from_numpy(np.array(panel[f])).to(dev) for f in INPUT_FIELDS]
    if layout == "pitched":
        ins = [pitched(x, T + 192 + (T & 1))[1] for x in ins]
    elif layout == "shifted":
        ins = [pitched(x, T + 192, shift=1)[1] for x in ins]
    return ins


def output_views(T, dev, layout, columns):
    """{column: (buffer, [S, T] view)}, every element SENTINEL"""
    blank = torch.empty((S, T), dtype=torch.float64, device=dev)
    pitch = {"contiguous": T, "padded": T + 192, "pitched": T + 192 + (T & 1), "shifted": T + 192}[layout]
    out = {}
    for c in columns:
        buf, view = pitched(blank, pitch, shift=1 if layout == "shifted" else 0)
        buf.fill_(SENTINEL)
        out[c] = (buf, view)
    return out


def run(ins, T, layout, columns=ENRICH_COLUMNS, params=None):
    """enrich into fresh outputs of the layout; the padding must stay untouched"""
    dev = ins[0].device
    outs = output_views(T, dev, layout, columns)
    got = engine.enrich(*ins, params=params, columns=columns, out={c: v for c, (_, v) in outs.items()})
    torch.cuda.synchronize()
    for c, (buf, view) in outs.items():
        written = torch.zeros_like(buf, dtype=torch.bool)
        shift = 1 if layout == "shifted" else 0
        written[shift:shift + S * view.stride(0)].view(S, view.stride(0))[:, :T] = True
        assert bool((buf[~written] == SENTINEL).all()), f"{c}: a store landed outside the [S, T] view ({layout}, T={T})"
    return {c: got[c].contiguous() for c in columns}


def run_generic(ins, T, layout, params=None):
    """all 14 columns through the generic kernels: two calls, each omitting one column"""
    a = run(ins, T, layout, columns=ENRICH_COLUMNS[:-1], params=params)
    b = run(ins, T, layout, columns=ENRICH_COLUMNS[1:], params=params)
    for c in ENRICH_COLUMNS[1:-1]:
        assert_same(a[c], b[c], f"{c} (generic, two calls)")
    return {**b, **a}


def assert_same(got, want, what):
    g, w = got.view(torch.int64), want.view(torch.int64)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        r, t = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at row {r} candle {t}: "
                             f"{float(got[r, t])!r} != {float(want[r, t])!r}")


def assert_all_same(got, want, what):
    for c in ENRICH_COLUMNS:
        assert_same(got[c], want[c], f"{c}, {what}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T", LENGTHS)
def test_hot_path_equals_generic_path(cuda, T, layout):
    ins = device_inputs(host_panel(T), cuda, layout)
    hot = run(ins, T, layout)
    assert_all_same(hot, run_generic(ins, T, layout), f"T={T}, {layout}: all 14 columns vs a call omitting one")


@pytest.mark.parametrize("T", [t for t in LENGTHS if t % 2 == 0])
def test_hot_path_equals_elementwise_path(cuda, T):
    """inputs and outputs moved by one element inside a larger buffer are
    8-byte aligned only: the element-wise loads and stores"""
    panel = host_panel(T)
    hot = run(device_inputs(panel, cuda, "contiguous"), T, "contiguous")
    slow = run(device_inputs(panel, cuda, "shifted"), T, "shifted")
    assert_all_same(hot, slow, f"T={T}: aligned vs misaligned rows")


def test_missing_row_rewrite_from_the_steady_loop(cuda):
    """a NaN and a +inf in the middle of an interior tile (the steady loop
    raises the row's flag; the row is recomputed after the walk)"""
    T, at = 4096, 2500
    clean = {k: v.copy() for k, v in host_panel(T).items()}
    assert all(np.isfinite(v).all() for v in clean.values())
    dirty = {k: v.copy() for k, v in clean.items()}
    dirty["close"][1, at] = np.nan
    dirty["volume"][3, at] = np.inf
    for layout in ("contiguous", "padded"):
        ins = device_inputs(dirty, cuda, layout)
        hot = run(ins, T, layout)
        assert_all_same(hot, run_generic(ins, T, layout), f"{layout}: rows with a NaN / +inf")
        base = run(device_inputs(clean, cuda, layout), T, layout)
        rows = [0, 2, 4]
        for c in ENRICH_COLUMNS:
            assert_same(hot[c][rows], base[c][rows], f"{c}, {layout}: clean rows beside the rewritten ones")
        assert bool(torch.isnan(hot["ma_7"][1, at:at + 7]).all()) and not bool(torch.isnan(hot["ma_7"][1, at + 7]))


def test_other_windows_keep_the_generic_kernel(cuda):
    """rsi_window = 6 is not the hot call: same values from the all-column
    call and from the calls omitting a column (both generic instantiations)"""
    T = 2832
    params = engine.IndicatorParams(rsi_window=6)
    ins = device_inputs(host_panel(T), cuda, "contiguous")
    got = run(ins, T, "contiguous", params=params)
    assert_all_same(got, run_generic(ins, T, "contiguous", params=params), "rsi_window=6")
    default = run(ins, T, "contiguous")
    assert not torch.equal(got["rsi"].view(torch.int64), default["rsi"].view(torch.int64))
    assert_same(got["mfi"], default["mfi"], "mfi is independent of rsi_window")
