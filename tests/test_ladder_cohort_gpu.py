"""GPU: process_cohort(grid_ladder=...) — LadderDeployer's decision for the
cohort's message, on the 15m frame's stream and its e15.bb_* columns —
against the stand-alone call and the numpy restatement, eager and as a
captured graph whose context tensors are refreshed in place."""

import functools

import numpy as np
import pytest
import torch

from tests import ladder_cases as lc
from tests.ladder_cases import ref

pytestmark = pytest.mark.gpu

STEP15 = 900_000
T0_MS = 1_776_000_000_000
NEW = ["gridladder.status"] + [f"gridladder.{k}" for k in ref.VALUES]


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cohort_inputs(S, T5, T15, seed=3):
    from binquant_amd.synth import numpy_panel

    p5, p15 = numpy_panel(S, T5, seed0=seed, edges=False), numpy_panel(S, T15, seed0=seed + 100, edges=False)
    ts15 = np.tile(T0_MS + np.arange(T15, dtype=np.int64) * STEP15, (S, 1))
    btc = 60000.0 * np.exp(np.cumsum(np.random.default_rng(5).normal(0.0, 0.001, T15)))
    cols = ("open", "high", "low", "close", "volume")
    return [dv(p5[k]) for k in cols] + [dv(p15[k]) for k in cols] + [dv(ts15), dv(ts15[0]), dv(btc)]


def context(S, seed, regime=ref.RANGE, policy=True, score=0.5):
    """One message's context, policy verdict and one snapshot entry per row (most rows pass every symbol gate)."""
    rng = np.random.default_rng(seed)
    rs = np.where(rng.random(S) < 0.8, rng.uniform(0.01, 0.3, S), rng.uniform(-0.2, 0.0, S))
    atr = rng.uniform(0.001, 0.04, S)
    atr[rng.random(S) < 0.1] = np.nan
    sym = dict(ok=rng.random(S) < 0.9, micro_regime=np.full(S, ref.RANGE, np.uint8),
               micro_transition=np.full(S, ref.NONE, np.uint8), above_ema20=rng.random(S) < 0.8,
               above_ema50=np.ones(S, bool), rs_vs_btc=rs, atr_pct=atr)
    return dict(market_regime=np.full(1, regime, np.int8), long_regime_score=np.full(1, score),
                ctx_ok=np.ones(1, bool), policy_ok=np.full(1, policy), sym=sym)


def on_device(c):
    ctx = dv(np.stack([c["market_regime"].astype(np.float64), c["long_regime_score"]]))
    return ctx, dv(c["ctx_ok"]), dv(c["policy_ok"]), {k: dv(v) for k, v in c["sym"].items()}


def refresh(dev, c):
    new = on_device(c)
    for a, b in zip(dev[:3], new[:3]):
        a.copy_(b)
    for k in dev[3]:
        dev[3][k].copy_(new[3][k])


def restated(c, close, frame):
    """The restatement on the cohort's own e15.bb_* (device tensors)."""
    p = dict(c, close=close.cpu().numpy(), **{k: v.cpu().numpy() for k, v in zip(lc.BB, frame)})
    return lc.ref_replay(p)


def test_cohort_outputs_equal_standalone_calls(cuda):
    """64 x 130 (5m) / 64 x 160 (15m): gridladder.* equal the stand-alone call's
    newest column on the cohort's own e15.bb_* and the restatement; without
    the keyword the dict's keys and values are the parent's (gates=True's
    ladder.* included)."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort

    S, T5, T15 = 64, 130, 160
    args = cohort_inputs(S, T5, T15)
    c = context(S, seed=8)
    dev = on_device(c)
    plain = process_cohort(*args, gates=True)
    parent_keys = list(plain)
    assert not any(k.startswith("gridladder.") for k in plain) and "ladder.stable" in plain
    full = process_cohort(*args, gates=True, grid_ladder=dev)
    torch.cuda.synchronize()
    assert [k for k in full if k not in plain] == NEW
    assert [k for k in full if k in plain] == parent_keys
    bare = process_cohort(*args, grid_ladder=dev)   # the keyword does not need gates=True
    assert [k for k in bare if k.startswith(("ladder.", "impulse."))] == []
    assert [k for k in bare if k.startswith("gridladder.")] == NEW
    for k in parent_keys:
        a, b = plain[k], full[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        a, b = torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)
        if k.startswith("h1.") and a.dim() == 2:   # bins past a row's count are left unwritten
            written = torch.arange(a.shape[1], device="cuda")[None, :] < plain["h1.bins"][:, None]
            a, b = a * written, b * written
        assert torch.equal(a, b), k
    assert full["gridladder.status"].dtype == torch.uint8
    frame = [full[f"e15.{k}"] for k in lc.BB]
    alone = signals.grid_ladder_entry(args[8], *frame, dev[0], dev[1], dev[2], sym=dev[3])
    want = restated(c, args[8], frame)
    for k in ("status",) + ref.VALUES:
        a, b = alone[k][:, -1].cpu().numpy(), full[f"gridladder.{k}"].cpu().numpy()
        assert a.shape == b.shape == (S,)
        assert lc.same_bits(a, b).all() and lc.same_bits(b, want[k][:, -1]).all(), k
    last = want["status"][:, -1]
    assert (last == ref.MICRO_REGIME).any() and (last == ref.RS_NOT_POSITIVE).any()
    assert ((last == ref.EMIT) | (last >= ref.BB_EXPANDING)).sum() >= S // 2   # most rows get to the frame's tests
    # the newest candle's verdict is the frame scan's
    walked = (last == ref.EMIT) | (last >= ref.BB_EXPANDING)
    assert ((last != ref.BB_EXPANDING)[walked] == full["ladder.stable"][:, -1].cpu().numpy()[walked]).all()
    none = process_cohort(*args, grid_ladder=(dev[0], None, None, None))   # no flags: present, allowed; no snapshot
    assert (none["gridladder.status"] == ref.MICRO_REGIME).all()


def test_cohort_graph_replay_equals_eager(cuda):
    """process_cohort(grid_ladder=...) captured once and replayed over three
    messages (a window sliding by one candle) at 8 rows x 100, the captured
    cohort tests' shape: the context, the policy verdict and the snapshot are
    device tensors refreshed in place between replays; gridladder.* equal
    eager calls' and the restatement."""
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline

    S, T5, W = 8, 100, 100
    full_args = cohort_inputs(S, T5, W + 3, seed=9)

    def window(e):
        a = list(full_args)
        for i in range(5, 11):   # the 15m panels and ts15
            a[i] = full_args[i][:, e - W:e].contiguous()
        a[11], a[12] = full_args[11][e - W:e].contiguous(), full_args[12][e - W:e].contiguous()
        return a

    dev = on_device(context(S, seed=1))
    fn = functools.partial(process_cohort, grid_ladder=dev)
    graph = CapturedPipeline(fn, *window(W))
    seen = []
    for e, kw in ((W + 1, {}), (W + 2, dict(policy=False)), (W + 3, dict(regime=0))):
        c = context(S, seed=e, **kw)
        refresh(dev, c)
        eager = {k: v.clone() for k, v in fn(*window(e)).items() if k.startswith(("gridladder.", "e15.bb_"))}
        got = graph(*window(e))
        torch.cuda.synchronize()
        assert [k for k in eager if k.startswith("gridladder.")] == NEW
        want = restated(c, window(e)[8], [eager[f"e15.{k}"] for k in lc.BB])
        for k in NEW:
            g = got[k].double().cpu().numpy()
            assert lc.same_bits(g, eager[k].double().cpu().numpy()).all(), (e, k)
            assert lc.same_bits(g, want[k[len("gridladder."):]][:, -1]).all(), (e, k)
        seen.append(got["gridladder.status"].cpu().numpy().copy())
    assert not np.isin(seen[0], (ref.POLICY, ref.NOT_RANGE, ref.NO_FRAME)).any()
    assert (seen[1] == ref.POLICY).all() and (seen[2] == ref.NOT_RANGE).all()
