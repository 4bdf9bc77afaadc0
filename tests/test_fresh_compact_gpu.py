"""GPU check of bq_panel_compact (engine.compact_panel): each row's present
candles — finite close; MarketStateStore drops a candle without one,
market_regime/market_state_store.py:84 — packed to the front in order,
against a numpy boolean-mask compaction. Values bit-equal; rank, n_present,
first_t exact; the tail repeats the last present candle (1.0 for an empty
row). Shapes cover one wave's tile (256 candles) on both sides of its edge,
rows that do not fill a workgroup (4 symbols) and more than one workgroup."""

import numpy as np
import pytest
import torch

from binquant_amd import engine

pytestmark = pytest.mark.gpu

TILE = 256


def _patterns(S, T, g):
    t = np.arange(T)
    run = np.ones((S, T), dtype=bool)
    run[:, 250:262] = False   # a run of absences across the tile edge (clipped to T)
    return {
        "all": np.ones((S, T), dtype=bool),
        "none": np.zeros((S, T), dtype=bool),
        "alternating": np.broadcast_to(t % 2 == 1, (S, T)) ^ (np.arange(S)[:, None] % 2 == 0),
        "one_per_tile": np.broadcast_to(t % TILE == min(37, T - 1), (S, T)),
        "random": g.random((S, T)) < 0.5,
        "edge_run": run,
    }


def _panel(S, T, g):
    c = 10.0 * np.exp(np.cumsum(g.normal(0, 0.01, (S, T)), axis=1))
    return c * (1 + g.uniform(0, 0.01, (S, T))), c * (1 - g.uniform(0, 0.01, (S, T))), c


def _expect(h, l, c):
    S, T = c.shape
    mask = np.isfinite(c)
    out = [np.ones((S, T)) for _ in range(3)]
    rank = np.where(mask, np.cumsum(mask, axis=1) - 1, -1).astype(np.int32)
    n = mask.sum(axis=1).astype(np.int32)
    first = np.where(n > 0, mask.argmax(axis=1), T).astype(np.int32)
    for s in range(S):
        for o, x in zip(out, (h, l, c)):
            v = x[s][mask[s]]
            o[s, :n[s]] = v
            if n[s]:
                o[s, n[s]:] = v[-1]
    return out, rank, n, first


def _check(h, l, c, dev_hlc=None):
    want, rank, n, first = _expect(h, l, c)
    d = dev_hlc or tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (h, l, c))
    got = engine.compact_panel(*d)
    for name, g_, w in zip(("high", "low", "close"), (got.high, got.low, got.close), want):
        np.testing.assert_array_equal(g_.cpu().numpy(), w, err_msg=name)
    np.testing.assert_array_equal(got.rank.cpu().numpy(), rank)
    np.testing.assert_array_equal(got.n_present.cpu().numpy(), n)
    np.testing.assert_array_equal(got.first_t.cpu().numpy(), first)
    assert int(got.n_invalid.sum().item()) == 0
    return got


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 256, 257, 700])
@pytest.mark.parametrize("S", [1, 3, 70])
def test_compact_equals_numpy_mask(cuda, S, T):
    g = np.random.default_rng(1000 * S + T)
    h, l, c = _panel(S, T, g)
    for name, present in _patterns(S, T, g).items():
        nan = np.where(present, 1.0, np.nan)
        _check(h * nan, l * nan, c * nan)


@pytest.mark.parametrize("S,T,pad", [(3, 65, 3), (70, 257, 1), (70, 700, 36)])
def test_compact_padded_row_stride(cuda, S, T, pad):
    """ld_in beyond T (odd and even pitches: the scalar and the 16-byte load paths)"""
    g = np.random.default_rng(S + T + pad)
    h, l, c = _panel(S, T, g)
    nan = np.where(g.random((S, T)) < 0.5, 1.0, np.nan)
    h, l, c = h * nan, l * nan, c * nan
    dev = tuple(torch.from_numpy(np.concatenate([x, np.full((S, pad), 7.0)], axis=1)).cuda()[:, :T] for x in (h, l, c))
    assert dev[0].stride(0) == T + pad
    _check(h, l, c, dev)


def test_compact_twice_is_bitwise_equal(cuda):
    g = np.random.default_rng(5)
    h, l, c = _panel(70, 700, g)
    nan = np.where(g.random((70, 700)) < 0.7, 1.0, np.nan)
    d = tuple(torch.from_numpy(x * nan).cuda() for x in (h, l, c))
    a, b = engine.compact_panel(*d), engine.compact_panel(*d)
    for x, y in ((a.high, b.high), (a.low, b.low), (a.close, b.close), (a.rank, b.rank)):
        assert torch.equal(x, y)


def test_invalid_candles_are_counted_and_rejected(cuda):
    g = np.random.default_rng(9)
    S, T = 5, 300
    h, l, c = _panel(S, T, g)
    c[1, 10] = np.nan
    h[1, 10] = l[1, 10] = np.nan          # an absent candle: fine
    # +-inf closes: invalid, treated as absent
    ci = c.copy()
    ci[2, 7] = np.inf
    ci[2, 260] = -np.inf
    d = tuple(torch.from_numpy(x).cuda() for x in (h, l, ci))
    with pytest.raises(ValueError, match=r"row 2 .*DeviceMarketStateStore"):
        engine.compact_panel(*d)
    got = engine.compact_panel(*d, validate=False)
    np.testing.assert_array_equal(got.n_invalid.cpu().numpy(), [0, 0, 2, 0, 0])
    np.testing.assert_array_equal(got.n_present.cpu().numpy(), [T, T - 1, T - 2, T, T])
    assert got.rank[2, 7].item() == -1 and got.rank[2, 260].item() == -1 and got.rank[2, 261].item() == 259
    # a present candle without a finite high / low: invalid (the store keeps such candles)
    hn, ln = h.copy(), l.copy()
    hn[3, 299] = np.nan
    ln[4, 0] = np.inf
    d = tuple(torch.from_numpy(x).cuda() for x in (hn, ln, c))
    with pytest.raises(ValueError, match="row 3"):
        engine.compact_panel(*d)
    got = engine.compact_panel(*d, validate=False)
    np.testing.assert_array_equal(got.n_invalid.cpu().numpy(), [0, 0, 0, 1, 1])
    np.testing.assert_array_equal(got.n_present.cpu().numpy(), [T, T - 1, T, T, T])
