"""engine.symbol_regime_panel's and MarketContextBatch.snapshot's argument
checks — every one a ValueError with its text written out, raised on the host
before anything is launched — and the O(T) host part of the snapshot
(batch.seen_columns) against a brute-force reading of the provider's rule."""

import re

import numpy as np
import pytest
import torch

from binquant_amd import _lib, engine
from binquant_amd.market_regime.batch import MarketContextBatch, PanelSnapshot, seen_columns
from binquant_amd.market_regime.regime import ContextBatch

S, T = 3, 8


def _feats(**over):
    f = {n: torch.zeros(S, T, dtype=torch.float64) for n in _lib.FEATURE_COLUMNS}
    f.update(over)
    return f


def _close():
    return torch.zeros(S, T, dtype=torch.float64)


def _raises(text, feats=None, close=None, **kw):
    with pytest.raises(ValueError, match=re.escape(text)):
        engine.symbol_regime_panel(_feats() if feats is None else feats, _close() if close is None else close, **kw)


def test_unknown_columns():
    _raises("symbol_regime_panel: unknown columns ['regime'] (known: ('ok', 'micro_regime', 'micro_transition', "
            "'above_ema20', 'above_ema50', 'rs_vs_btc', 'micro_regime_strength', 'micro_transition_strength', "
            "'trend_score', 'atr_pct', 'bb_width'))", columns=("ok", "regime"))


def test_shapes_dtypes_strides():
    _raises("close: expected [S, T] with unit stride along T", close=torch.zeros(T, dtype=torch.float64))
    f = _feats()
    del f["ema50"]
    _raises("feats: missing ['ema50'] (expected ('return_pct', 'ema20', 'ema50', 'trend_score', 'atr_pct', "
            "'bb_width'))", feats=f)
    _raises("atr_pct: expected dtype float64, got torch.float32", feats=_feats(atr_pct=torch.zeros(S, T)))
    _raises("ema20: shape (3, 7) != (3, 8)", feats=_feats(ema20=torch.zeros(S, T - 1, dtype=torch.float64)))
    _raises("close: expected dtype float64, got torch.float32", close=torch.zeros(S, T))
    _raises("trend_score: expected [S, T] with unit stride along T",
            feats=_feats(trend_score=torch.zeros(T, S, dtype=torch.float64).t()))
    _raises("close: expected [S, T] with unit stride along T", close=torch.zeros(T, S, dtype=torch.float64).t())
    _raises("feature columns must share one row stride",
            feats=_feats(bb_width=torch.zeros(S, T + 4, dtype=torch.float64)[:, :T]))
    _raises("rank: expected an int32 tensor of shape (3, 8) with unit stride along T",
            rank=torch.zeros(S, T, dtype=torch.int64))
    _raises("rank: expected an int32 tensor of shape (3, 8) with unit stride along T",
            rank=torch.zeros(T, S, dtype=torch.int32).t())


def test_index_ranges():
    _raises("at: expected a 1-D int32 / int64 tensor", at=np.zeros((2, 2), dtype=np.int64))
    _raises("at: expected a 1-D int32 / int64 tensor", at=np.zeros(4))
    _raises("at: values in -1..7 (context columns), got 0..8", at=np.array([0, 8]))
    _raises("at: values in -1..7 (context columns), got -2..3", at=torch.tensor([-2, 3]))
    _raises("prev: expected a 1-D int32 / int64 tensor of shape (8,)", prev=np.zeros(9, dtype=np.int64))
    _raises("prev: expected a 1-D int32 / int64 tensor of shape (2,)", at=np.array([1, 2]), prev=np.zeros(3, dtype=int))
    _raises("prev: values in -2..7 (context columns), got -3..0", prev=np.array([-3] + [0] * 7))
    _raises("prev: values in -2..7 (context columns), got 0..8", prev=np.array([8] + [0] * 7))


def test_btc_and_seed():
    _raises("btc_return: expected a float64 tensor of shape (8,)", btc_return=torch.zeros(T))
    _raises("btc_return: expected a float64 tensor of shape (8,)", btc_return=torch.zeros(T + 1, dtype=torch.float64))
    _raises("btc_row: expected None or a row in 0..2, got 3", btc_row=3)
    _raises("btc_row: expected None or a row in 0..2, got -1", btc_row=-1)
    text = "seed: expected (micro_regime int8, micro_regime_strength float64) contiguous tensors of shape (3,)"
    _raises(text, seed=(torch.zeros(S, dtype=torch.int8),))
    _raises(text, seed=(torch.zeros(S, dtype=torch.uint8), torch.zeros(S, dtype=torch.float64)))
    _raises(text, seed=(torch.zeros(S, dtype=torch.int8), torch.zeros(S + 1, dtype=torch.float64)))


def test_host_tensors_have_no_path():
    _raises("symbol_regime_panel: expected CUDA tensors (no CPU path)")


def _batch(valid, feats_cols, rank=None):
    n = len(valid)
    cb = ContextBatch(timestamp=1000 + 900 * np.arange(n, dtype=np.int64), valid=np.asarray(valid, bool),
                      fields=dict(btc_present=np.ones(n, bool), btc_return=np.zeros(n)))
    feats = {k: torch.zeros(S, feats_cols, dtype=torch.float64) for k in _lib.FEATURE_COLUMNS}
    return MarketContextBatch(contexts=cb, features=feats, partial=torch.zeros(n, 10, dtype=torch.float64), rank=rank)


def test_snapshot_after_a_fused_build():
    b = _batch([True] * T, 1)   # keep_features=False: the last timestamp's row only
    with pytest.raises(ValueError, match=re.escape(
            "snapshot: a fused context build (keep_features=False) keeps no feature columns")):
        b.snapshot(_close())


def test_snapshot_checks():
    b = _batch([True] * T, T, rank=torch.zeros(S, T, dtype=torch.int32))
    with pytest.raises(ValueError, match=re.escape(
            "snapshot: a fresh build needs compact_close, the packed close of its features")):
        b.snapshot(_close())
    b = _batch([True] * T, T)
    with pytest.raises(ValueError, match=re.escape("times: expected a 1-D int64 array of candle close times")):
        b.snapshot(_close(), times=np.zeros(4))
    b.contexts.timestamp = b.contexts.timestamp[::-1].copy()
    with pytest.raises(ValueError, match=re.escape("snapshot: times= needs ascending context timestamps")):
        b.snapshot(_close(), times=np.zeros(4, dtype=np.int64))


def _brute(valid, ts, carry, times, seeded):
    """The provider's rule read literally, one candle at a time."""
    at, prev = [], []
    for time in (ts if times is None else times):
        if carry:
            seen = [j for j in range(len(valid)) if valid[j] and ts[j] <= time]
        else:
            seen = [j for j in range(len(valid)) if valid[j] and ts[j] == time]
        j = seen[-1] if seen else -1
        earlier = [i for i in range(len(valid)) if valid[i] and i < j]
        at.append(j)
        prev.append(-1 if j < 0 else earlier[-1] if earlier else (-2 if seeded else -1))
    return np.array(at), np.array(prev)


@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("seeded", [False, True])
def test_seen_columns(carry, seeded):
    g = np.random.default_rng(5)
    for n in (0, 1, 2, 40):
        valid = g.random(n) < 0.6
        ts = 1000 + 900 * np.arange(n, dtype=np.int64)
        at, prev = seen_columns(valid, ts, carry=carry, seeded=seeded)
        wa, wp = _brute(valid, ts, carry, None, seeded)
        np.testing.assert_array_equal(at, wa.astype(np.int64).reshape(-1))
        np.testing.assert_array_equal(prev, wp.astype(np.int64).reshape(-1))
        # a frame on a three-times finer grid, starting before the first context
        times = 400 + 300 * np.arange(3 * n + 4, dtype=np.int64)
        at, prev = seen_columns(valid, ts, carry=carry, times=times, seeded=seeded)
        wa, wp = _brute(valid, ts, carry, times, seeded)
        np.testing.assert_array_equal(at, wa)
        np.testing.assert_array_equal(prev, wp)


def test_panel_snapshot_host_views():
    n = 6
    cb = ContextBatch(
        timestamp=1000 + 900 * np.arange(n, dtype=np.int64), valid=np.array([0, 1, 1, 0, 1, 1], bool),
        fields=dict(market_stress_score=np.arange(n) / 10.0, regime_is_transitioning=np.array([0, 1, 0, 0, 1, 0], bool),
                    market_regime=np.array(["RANGE", "TREND_UP", "RANGE", "RANGE", "HIGH_STRESS", "RANGE"], dtype=object),
                    regime_stable_since=np.array([None, 1900, 2800, None, 4600, 5500], dtype=object),
                    fresh_count=np.arange(n, dtype=np.int64)))
    at, _ = seen_columns(cb.valid, cb.timestamp)
    code = torch.tensor([[0, 255, 4]], dtype=torch.uint8)
    snap = PanelSnapshot(contexts=cb, at=at, columns={"ok": torch.tensor([[1, 0, 1]], dtype=torch.uint8),
                                                      "micro_regime": code, "micro_transition": code},
                         device=torch.device("cpu"))
    assert snap.ok.tolist() == [False, True, True, True, True, True]
    ctx = snap.ctx(_lib.RF_CTX_ROWS + ("confidence", "fresh_count")).numpy()
    assert np.isnan(ctx[:, 0]).all()
    np.testing.assert_array_equal(ctx[:, 1:], [[1, 0, 0, 1, 0], [0.1, 0.2, 0.2, 0.4, 0.5], [0, 2, 2, 3, 2],
                                               [1, 1, 1, 1, 1], [1, 2, 2, 4, 5]])
    assert snap.timestamp.tolist() == [-1, 1900, 2800, 2800, 4600, 5500]
    assert snap.regime_stable_since.tolist() == [-1, 1900, 2800, 2800, 4600, 5500]
    with pytest.raises(ValueError, match=re.escape("ctx: unknown row 'previous_market_regime' (known: ['confidence', "
                                                   "'fresh_count', 'market_regime', 'market_stress_score', "
                                                   "'regime_is_transitioning'])")):
        snap.ctx(("previous_market_regime",))
    u = snap.sym(("ok", "micro_regime"))
    assert u["ok"].dtype == torch.uint8 and u["micro_regime"].tolist() == [[0, 255, 4]]
    i = snap.sym(("ok", "micro_regime", "micro_transition"), none="int8")
    assert i["ok"].dtype == torch.bool and i["micro_regime"].dtype == torch.int8
    assert i["micro_transition"].tolist() == [[0, -1, 4]]
    with pytest.raises(ValueError, match=re.escape("sym: none is 'uint8' (_lib.MR_NONE) or 'int8' (negative), got 'i8'")):
        snap.sym(("ok",), none="i8")
    with pytest.raises(ValueError, match=re.escape("sym: ['atr_pct'] not among the snapshot's columns ('ok', "
                                                   "'micro_regime', 'micro_transition')")):
        snap.sym(("ok", "atr_pct"))
