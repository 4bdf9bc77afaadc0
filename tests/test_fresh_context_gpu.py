"""GPU parity of the fresh panel context build — market_context_batch(fresh=True):
bq_panel_compact, bq_market_features on the compacted panel,
bq_breadth_partial_fresh, one all-reduce, host scoring — for panels with
late listings, halts, delistings and missing candles, against

* the reference itself: MarketStateStore(30) + LiveMarketContextAccumulator
  fed the same candles (tests/golden/make_golden_fresh.py; fresh_panel.npz,
  fresh_context.json) — which contexts exist, every field, the regime labels
  and transitions, and per-symbol rows at three timestamps;
* the oracle restatement of _compute_symbol_features over the last max_bars
  present candles of every fresh symbol, at sampled timestamps;
* the dense kernels when every candle is present (the same templated kernels,
  so the same reduction order: bit-equal at every T);
and checks that absent candles poison nothing and that a launch repeats
bit for bit."""

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from binquant_amd import engine
from binquant_amd._lib import FEATURE_COLUMNS
from binquant_amd.market_regime.batch import market_context_batch
from binquant_amd.synth import numpy_panel
from oracle import market_ref
from tests.util import assert_close

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
SKIP = ("symbol_features", "metadata", "btc_symbol", "confidence", "is_provisional", "timestamp")


def _cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs)


def _fresh_partials(h, l, c, M):
    comp = engine.compact_panel(h, l, c)
    feats = engine.market_features(comp.high, comp.low, comp.close, max_bars=M)
    return engine.breadth_partial_fresh(comp, feats), comp, feats


# ---- the reference's own contexts -------------------------------------------------

@pytest.fixture(scope="module")
def golden(cuda):
    meta = json.loads((G / "fresh_context.json").read_text())
    panel = np.load(G / "fresh_panel.npz")
    h, l, c = _cuda(panel["high"], panel["low"], panel["close"])
    b = meta["symbols"].index(meta["btc"])
    batch = market_context_batch(h, l, c, (h[b:b + 1], l[b:b + 1], c[b:b + 1]), max_bars=meta["max_bars"],
                                 timestamps=np.array(meta["timestamps"]), fresh=True)
    return meta, batch, c, b


def test_fresh_contexts_match_reference_golden(golden):
    meta, batch, _, _ = golden
    want_all = meta["contexts"]
    assert len(want_all) == 120
    exists = np.array([w is not None for w in want_all])
    np.testing.assert_array_equal(batch.contexts.valid, exists)
    idx = np.flatnonzero(exists)
    got_all = [batch.context_at(int(i)) for i in idx]
    for k, v0 in want_all[idx[0]].items():
        if k in SKIP:
            continue
        want = [want_all[i][k] for i in idx]
        got = [g[k] for g in got_all]
        if all(isinstance(v, float) for v in want):
            assert_close(np.array(got, dtype=float), np.array(want), k)
        else:   # counts, total_tracked_symbols, flags, regime labels, transitions, stable-since
            assert got == want, (k, [(int(i), a, b) for i, a, b in zip(idx, got, want) if a != b][:5])
    assert len({w["total_tracked_symbols"] for w in want_all if w}) >= 5
    # stale BTC: contexts exist where BTC has no candle, with its last features
    for t in meta["stale_btc"]:
        assert batch.context_at(t)["btc_present"] is True


@pytest.mark.parametrize("t", [50, 71, 119])
def test_fresh_symbol_features_match_reference_golden(golden, t):
    meta, batch, close, b = golden
    want = meta["symbol_features"][str(t)]
    ctx = batch.context_at(t)
    got = batch.symbol_features_at(t, close, ctx["btc_return"] if ctx["btc_present"] else None, btc_index=b)
    syms = meta["symbols"]
    rows = [syms.index(s) for s in want]
    # exactly the reference's symbols have features: fresh at t with >= 2 candles
    np.testing.assert_array_equal(np.flatnonzero(~np.isnan(got["return_pct"])), sorted(rows))
    for k in ("close", "return_pct", "ema20", "ema50", "trend_score", "relative_strength_vs_btc", "atr_pct",
              "bb_width", "micro_regime_strength"):
        assert_close(got[k][rows], np.array([want[s][k] for s in want]), f"{k}@{t}")
    for k in ("above_ema20", "above_ema50", "micro_regime"):
        assert list(got[k][rows]) == [want[s][k] for s in want], k


# ---- the oracle on a random sparse panel --------------------------------------------

def _sparse_panel(S, T, seed):
    g = np.random.default_rng(seed)
    p = numpy_panel(S, T, seed0=seed, edges=False)
    present = g.random((S, T)) < g.uniform(0.3, 1.0, S)[:, None]
    for s in range(0, S, 7):
        present[s, :g.integers(1, T - 1)] = False   # late listings
    present[5] = False                              # never present
    present[6, 300:] = False                        # delisted
    nan = np.where(present, 1.0, np.nan)
    return p["high"] * nan, p["low"] * nan, p["close"] * nan, present


@pytest.fixture(scope="module")
def sparse(cuda):
    h, l, c, present = _sparse_panel(70, 700, 31337)
    return h, l, c, present, _cuda(h, l, c)


@pytest.mark.parametrize("M", [15, 400])
def test_fresh_partials_match_oracle(sparse, M):
    h, l, c, present, dev = sparse
    S, T = c.shape
    part, _, _ = _fresh_partials(*dev, M)
    part = part.cpu().numpy()
    assert np.isfinite(part).all()
    first = np.where(present.any(axis=1), present.argmax(axis=1), T)
    np.testing.assert_array_equal(part[:, 9], (first[:, None] <= np.arange(T)[None, :]).sum(axis=0))
    packed = [tuple(x[s][present[s]] for x in (h, l, c)) for s in range(S)]   # the compaction, on the host
    rank = np.cumsum(present, axis=1) - 1
    ts = [0, 1, 2, 255, 256, 257, 511, 512, 699]
    ts += [int(t) for t in np.random.default_rng(M).permutation(T) if t not in ts][:40 - len(ts)]
    assert len(set(ts)) == 40
    for t in sorted(ts):
        feats = []
        for s in np.flatnonzero(present[:, t]):
            k = rank[s, t]
            lo = max(0, k - M + 1)
            f = market_ref.symbol_features(*(x[lo:k + 1] for x in packed[s]))
            if f is not None:
                feats.append(f)
        if not feats:
            np.testing.assert_array_equal(part[t, :9], 0.0)
            continue
        f = {k: np.array([x[k] for x in feats]) for k in feats[0]}
        # exact counts need every close clear of its EMAs (true of this seed)
        assert not any((np.abs(f["close"] - f[e]) <= 1e-9 * np.abs(f["close"])).any() for e in ("ema20", "ema50"))
        wp = market_ref.partials_from_features(f)
        np.testing.assert_array_equal(part[t, :5], wp[:5], err_msg=f"counts@{t}")
        for i, k in ((5, "return_pct"), (6, "trend_score"), (7, "atr_pct"), (8, "bb_width")):
            mag = np.abs(f[k]).sum()
            assert abs(part[t, i] - wp[i]) <= 1e-9 * mag + 1e-300, (t, k, part[t, i], wp[i])


# ---- every candle present: the dense kernels -------------------------------------------

@pytest.mark.parametrize("T", [300, 60])
def test_all_present_equals_dense(cuda, T):
    S, M = 70, 400
    p = numpy_panel(S, T, seed0=909 + T, edges=False)
    h, l, c = _cuda(p["high"], p["low"], p["close"])
    f = engine.market_features(h, l, c, max_bars=M)
    want = engine.breadth_partial(c, f).cpu().numpy()
    got, comp, fc = _fresh_partials(h, l, c, M)
    got = got.cpu().numpy()
    assert torch.equal(comp.close, c) and torch.equal(comp.rank, torch.arange(T, device=c.device).expand(S, T).int())
    np.testing.assert_array_equal(got[:, 9], float(S))
    # T > 256: breadth_kernel<dense / fresh>, T <= 256: breadth_small_kernel<dense / fresh>;
    # either pair shares its walk and its combine, so the order is the dense one exactly
    np.testing.assert_array_equal(got[:, :9], want[:, :9])


# ---- absent candles poison nothing; launches repeat ---------------------------------------

@pytest.mark.parametrize("T", [300, 60])
def test_nan_closes_do_not_poison_and_empty_timestamp_is_invalid(cuda, T):
    S = 70
    g = np.random.default_rng(T)
    p = numpy_panel(S, T, seed0=4 + T, edges=False)
    present = g.random((S, T)) < 0.97
    present[:, 40] = False                 # nobody has a candle here
    nan = np.where(present, 1.0, np.nan)
    h, l, c = _cuda(p["high"] * nan, p["low"] * nan, p["close"] * nan)
    batch = market_context_batch(h, l, c, (h[:1], l[:1], c[:1]), max_bars=400, fresh=True)
    part = batch.partial.cpu().numpy()
    assert np.isfinite(part).all()
    assert part[40, 0] == 0 and not batch.contexts.valid[40] and batch.context_at(40) is None
    assert batch.contexts.valid[41:].any()
    with pytest.raises(ValueError, match="keep_features"):
        market_context_batch(h, l, c, (h[:1], l[:1], c[:1]), fresh=True, keep_features=False)
    # an explicit total_tracked still overrides the kernel's per-timestamp count
    forced = market_context_batch(h, l, c, (h[:1], l[:1], c[:1]), max_bars=400, fresh=True, total_tracked=1000)
    assert not forced.contexts.valid.any()
    assert (forced.contexts.fields["total_tracked_symbols"] == 1000).all()


@pytest.mark.parametrize("T", [700, 256])
def test_two_launches_are_bitwise_equal(sparse, T):
    _, _, _, _, dev = sparse
    h, l, c = (x[:, :T].contiguous() for x in dev)
    comp = engine.compact_panel(h, l, c)
    feats = engine.market_features(comp.high, comp.low, comp.close, max_bars=30)
    a = engine.breadth_partial_fresh(comp, feats)
    b = engine.breadth_partial_fresh(comp, feats, out=torch.full_like(a, -1.0))
    assert torch.equal(a, b)
    assert all(n in feats for n in FEATURE_COLUMNS)
