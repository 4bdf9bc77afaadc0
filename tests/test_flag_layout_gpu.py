"""The bool [S, T] flag panels of the five entries that take them
(top_gainer_entry, sweep_select, retest_replay, spike_frames,
spike_fade_replay) in two layouts the argument layer has to handle: a view
whose stride along T is not 1 (a transposed [T, S] tensor: copied) and a
column slice of a wider tensor (row pitch > T: read in place). Every output,
carried state included, is bit-equal to the call with contiguous flags.

S = 3, T = 130: two 64-candle steps and a tail, past the 56-candle history
gates of the top-gainer and sweep entries. spike_frames' wide case is
tests/test_spikeframes_gpu.py::test_padded_row_pitch."""

import numpy as np
import pytest
import torch

from tests import retest_cases as rc
from tests import spikefade_cases as fc
from tests import spikeframes_cases as mc
from tests import sweep_cases as wc
from tests import topgainer_cases as tc

pytestmark = pytest.mark.gpu

S, T = 3, 130


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(x):
    """[S, T] with strides (1, S)."""
    v = x.t().contiguous().t()
    assert tuple(v.shape) == tuple(x.shape) and v.stride(1) == x.shape[0] != 1
    return v


def wide(x):
    """Columns 5 .. 5 + T of a [S, T + 37] buffer of ones."""
    buf = torch.ones((x.shape[0], x.shape[1] + 37), dtype=x.dtype, device=x.device)
    v = buf[:, 5:5 + x.shape[1]]
    v.copy_(x)
    assert v.stride(1) == 1 and v.stride(0) == x.shape[1] + 37
    return v


LAYOUTS = {"strided": strided, "wide": wide}


def flat(res):
    """Every tensor of a result (tuples and dicts walked in order)."""
    if isinstance(res, torch.Tensor):
        return [res]
    if isinstance(res, dict):
        res = list(res.values())
    return [t for x in res if x is not None for t in flat(x)]


def assert_same_bits(got, want):
    got, want = flat(got), flat(want)
    assert len(got) == len(want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, i
        if g.dtype == torch.float64:
            g, w = g.contiguous().view(torch.int64), w.contiguous().view(torch.int64)
        assert torch.equal(g, w), f"output {i}"


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_top_gainer_risk_ok(cuda, layout):
    from binquant_amd import _lib, engine

    q = tc.injected_panel(S, T, seed=36, nan_rate=0.0)   # a confirmation in each row, one of them risk-rejected
    cols = [dv(q[k]) for k in (*tc.INPUTS, "quote_volume", "atr")]
    risk = dv(q["risk_ok"])
    want = engine.top_gainer_entry(*cols, risk_ok=risk)
    assert_same_bits(engine.top_gainer_entry(*cols, risk_ok=LAYOUTS[layout](risk)), want)
    st = want[0]
    assert int((st == 0).sum()) >= 1 and int((st == _lib.TGE_REASONS.index("risk_rejected")).sum()) >= 1


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_sweep_flags(cuda, layout):
    from binquant_amd import _lib, engine

    c, cross, route = wc.planted_columns(S, T, seed=5, density=0.3)
    cols = [dv(c[k]) for k in _lib.SW_COLUMNS]
    cross, route = dv(cross), dv(route)
    want = engine.sweep_select(cols, cross, route_ok=route)
    lay = LAYOUTS[layout]
    assert_same_bits(engine.sweep_select(cols, lay(cross), route_ok=lay(route)), want)
    assert_same_bits(engine.sweep_select(cols, lay(cross), route_ok=route), want)   # each flag on its own pitch
    st = want[0]
    assert int((st == 0).sum()) >= 5 and int((st == _lib.SW_REASONS.index("no_score_cross")).sum()) >= 5
    assert int((st == _lib.SW_REASONS.index("route_refused")).sum()) >= 1


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_retest_flags(cuda, layout):
    from binquant_amd import engine

    p = rc.edge_panel(T, seed=9)
    rows = slice(2, 2 + S)   # the dense-leader rows and the one with time gaps
    cols = [dv(p[k][rows]) for k in rc.COLS + ("ema", "open_time")]
    leader, risk = dv(p["leader"][rows]), dv(p["risk_ok"][rows])

    def run(leader, risk):
        state = (torch.zeros(S, dtype=torch.uint8, device="cuda"), torch.zeros(S, dtype=torch.int64, device="cuda"),
                 torch.full((S,), float("nan"), dtype=torch.float64, device="cuda"))
        return engine.retest_replay(*cols, leader, risk, state=state, **rc.EDGE_PARAMS), state

    want = run(leader, risk)
    lay = LAYOUTS[layout]
    assert_same_bits(run(lay(leader), lay(risk)), want)
    assert_same_bits(run(lay(leader), risk), want)   # one flag copied or padded: both end on one pitch
    ev = want[0][0]
    for code in (rc.ref.RT_EVENTS.index("watch_set"), rc.ref.RT_EVENTS.index("risk_blocked"),
                 rc.ref.RT_EVENTS.index("candidate")):
        assert int((ev == code).sum()) >= 1, code


def test_spike_frames_flags_strided(cuda):
    from binquant_amd import _lib, engine, strategies

    p = mc.synth_panel(S, T, seed=3)
    cols = strategies.spike_frame_columns(*(dv(p[k]) for k in ("open", "close", "volume")))
    par = strategies.SpikeParams()
    want = engine.spike_frames(cols, par)
    got = engine.spike_frames({k: strided(x) if k in _lib.SPIKE_FRAMES_IN_B else x for k, x in cols.items()}, par)
    assert_same_bits(got, want)
    one = engine.spike_frames({**cols, "upward": strided(cols["upward"])}, par)   # one flag copied: one pitch for all
    assert_same_bits(one, want)
    assert bool(want["label_pre"].any()) and bool(want["upward"].any()) and bool(want["downward"].any())


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_spike_fade_flags(cuda, layout):
    from binquant_amd import engine

    p = fc.edge_panel(S, T, seed=21)
    cols = [dv(p[k]) for k in fc.COLS + ("open_time",)]
    flags = [dv(p[k]) for k in ("source_ok", "src_market", "fail_market")]

    def run(source, src_m, fail_m):
        state = tuple(dv(x) for x in fc.idle_state(S))
        return engine.spike_fade_replay(*cols, source, src_m, fail_m, state=state), state

    want = run(*flags)
    lay = LAYOUTS[layout]
    assert_same_bits(run(*(lay(x) for x in flags)), want)
    assert_same_bits(run(lay(flags[0]), flags[1], lay(flags[2])), want)   # source_ok on its own pitch, the gates on one
    ev = want[0][0]
    for code in (fc.ref.FS_EVENTS.index("source_set"), fc.ref.FS_EVENTS.index("candidate"),
                 fc.ref.FS_EVENTS.index("cleared")):
        assert int((ev == code).sum()) >= 1, code
