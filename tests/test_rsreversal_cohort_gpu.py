"""GPU: process_cohort(rs_reversal=...) — RelativeStrengthReversalRange's
decision for the cohort's message, on the 15m frame's stream — against the
stand-alone call and the numpy restatement, eager and as a captured graph."""

import functools

import numpy as np
import pytest
import torch

from tests import rsreversal_cases as rc
from tests.rsreversal_cases import pg, ref

pytestmark = pytest.mark.gpu

STEP15 = pg.STEP_MS
NEW = ["rsr.status", "rsr.volume_floor"]


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cohort_inputs(S, T5, T15, seed=3):
    """process_cohort's positional inputs; the 15m volume rounded to one decimal (ties with the floor)."""
    from binquant_amd.synth import numpy_panel

    p5, p15 = numpy_panel(S, T5, seed0=seed, edges=False), numpy_panel(S, T15, seed0=seed + 100, edges=False)
    p15 = dict(p15, volume=np.round(p15["volume"] / p15["volume"].mean() * 40.0, 1))
    ts15 = np.tile(pg.T0_MS + np.arange(T15, dtype=np.int64) * STEP15, (S, 1))
    btc = 60000.0 * np.exp(np.cumsum(np.random.default_rng(5).normal(0.0, 0.001, T15)))
    cols = ("open", "high", "low", "close", "volume")
    return [dv(p5[k]) for k in cols] + [dv(p15[k]) for k in cols] + [dv(ts15), dv(ts15[0]), dv(btc)], p15["volume"]


def context(S, seed):
    """One context (the message's) and one snapshot entry per row."""
    rng = np.random.default_rng(seed)
    rs = np.where(rng.random(S) < 0.7, rng.uniform(0.051, 0.3, S), rng.uniform(-0.2, 0.05, S))
    return dict(context_ok=np.ones(1, bool), market_regime=np.full(1, ref.RANGE, np.int8),
                average_return=np.full(1, -0.03), features_ok=rng.random(S) < 0.85, rs=rs)


def test_cohort_outputs_equal_standalone_calls(cuda):
    """40 x 130 (5m) / 40 x 120 (15m), the eager cohort tests' shape: rsr.*
    equal the stand-alone call's newest column and the restatement; without the
    keyword the dict's keys and values are the parent's."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort

    S, T5, T15 = 40, 130, 120
    args, vol = cohort_inputs(S, T5, T15)
    c = context(S, seed=8)
    dev = tuple(dv(c[k]) for k in rc.CTX)
    plain = process_cohort(*args)
    parent_keys = list(plain)
    assert not any(k.startswith("rsr.") for k in plain)
    full = process_cohort(*args, rs_reversal=dev)
    torch.cuda.synchronize()
    assert [k for k in full if k not in plain] == NEW
    assert [k for k in full if k in plain] == parent_keys
    for k in parent_keys:
        a, b = plain[k], full[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        a, b = torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)
        if k.startswith("h1.") and a.dim() == 2:   # bins past a row's count are left unwritten
            written = torch.arange(a.shape[1], device="cuda")[None, :] < plain["h1.bins"][:, None]
            a, b = a * written, b * written
        assert torch.equal(a, b), k
    assert full["rsr.status"].dtype == torch.uint8 and full["rsr.volume_floor"].dtype == torch.float64
    alone = signals.rs_reversal_entry(args[9], *dev)
    want = rc.ref_replay(dict(c, volume=vol))
    for k, name in (("status", "rsr.status"), ("volume_floor", "rsr.volume_floor")):
        a, b = alone[k][:, -1].cpu().numpy(), full[name].cpu().numpy()
        assert a.shape == b.shape == (S,)
        assert rc.same_value(a, b).all() and rc.same_value(b, want[k][:, -1]).all(), k
    last = want["status"][:, -1]
    assert (last == ref.EMIT).any() and (last == ref.DEAD_TAPE).any() and (last == ref.RS_INSUFFICIENT).any()
    none = process_cohort(*args, rs_reversal=(None, dev[1], dev[2], None, dev[4]))   # both flags absent: present
    assert not (none["rsr.status"] == ref.NO_FEATURES).any() and not (none["rsr.status"] == ref.NO_CONTEXT).any()


def test_cohort_graph_replay_equals_eager(cuda):
    """process_cohort(rs_reversal=...) captured once and replayed over three
    messages (a window sliding by one candle) at 8 rows x 100 (5m), the
    captured cohort tests' shape, with a 15m window of 100 candles (the method
    needs 96 to reach the floor): the context and the snapshot are device
    tensors updated in place between replays; rsr.* equal eager calls' and the
    restatement."""
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline

    S, T5, W = 8, 100, 100
    full_args, vol = cohort_inputs(S, T5, W + 3, seed=9)

    def window(e):
        a = list(full_args)
        for i in range(5, 11):   # the 15m panels and ts15
            a[i] = full_args[i][:, e - W:e].contiguous()
        a[11], a[12] = full_args[11][e - W:e].contiguous(), full_args[12][e - W:e].contiguous()
        return a

    c = context(S, seed=1)
    dev = {k: dv(c[k]) for k in rc.CTX}
    fn = functools.partial(process_cohort, rs_reversal=tuple(dev[k] for k in rc.CTX))
    graph = CapturedPipeline(fn, *window(W))
    seen = []
    for e, regime, avg in ((W + 1, ref.RANGE, -0.03), (W + 2, ref.RANGE, -0.02), (W + 3, ref.RANGE, float("nan"))):
        c = dict(context(S, seed=e), market_regime=np.full(1, regime, np.int8), average_return=np.full(1, avg))
        for k in rc.CTX:
            dev[k].copy_(dv(c[k]))
        want = {k: v.clone() for k, v in fn(*window(e)).items() if k.startswith("rsr.")}
        got = graph(*window(e))
        torch.cuda.synchronize()
        assert list(want) == NEW
        alone = rc.ref_replay(dict(c, volume=vol[:, e - W:e]))
        for k in NEW:
            g = got[k].double().cpu().numpy()
            assert rc.same_value(g, want[k].double().cpu().numpy()).all(), (e, k)
            assert rc.same_value(g, alone[k[4:]][:, -1]).all(), (e, k)
        seen.append(got["rsr.status"].cpu().numpy().copy())
    assert (seen[1] == ref.MARKET_NOT_WEAK).all()   # exactly the limit
    assert len({s.tobytes() for s in seen}) == 3    # the messages differ
    assert any((s == ref.EMIT).any() for s in seen) and any((s == ref.DEAD_TAPE).any() for s in seen)
