"""The join of the panel context build and the panel entries: on the regime
fixture's panel, signals.range_fade_entry and signals.grid_ladder_entry
replayed over all candles from MarketContextBatch.snapshot's device tensors
equal the same entries fed tensors assembled on the host, one timestamp at a
time, from context_at / symbol_features_at with the transitions of
regime.annotate_symbols under the reference's predecessor rule (a symbol's
entry in the context stored immediately before the seen one)."""

import numpy as np
import pytest
import torch

from binquant_amd import _lib, engine, signals
from binquant_amd.market_regime.batch import market_context_batch
from binquant_amd.market_regime.regime import annotate_symbols
from tests import regime_panel_ref as ref

pytestmark = pytest.mark.gpu
NONE = _lib.MR_NONE
KEYS = ("ok", "micro_regime", "micro_transition", "above_ema20", "above_ema50", "rs_vs_btc", "atr_pct", "bb_width")


@pytest.fixture(scope="module")
def joined(cuda):
    fx = ref.fixture()
    o, h, l, c, present = ref.gen.build_panel()
    S, T = c.shape
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    nan = np.where(present, 1.0, np.nan)
    hm, lm, cm = dev(h * nan), dev(l * nan), dev(c * nan)
    b = ref.gen.BTC
    batch = market_context_batch(hm, lm, cm, (hm[b:b + 1], lm[b:b + 1], cm[b:b + 1]), max_bars=int(fx["max_bars"]),
                                 timestamps=fx["timestamps"], fresh=True)
    # the strategies' frame: the walks themselves, enriched
    px = {k: dev(v) for k, v in dict(open=o, high=h, low=l, close=c).items()}
    px["volume"] = dev(np.random.default_rng(1).uniform(1.0, 2.0, (S, T)))
    ind = engine.enrich(px["open"], px["high"], px["low"], px["close"], px["volume"])
    snap = batch.snapshot(cm, btc_index=b, carry=True)

    # ---- the host loop the snapshot replaces ----
    valid = batch.contexts.valid
    rows = sorted(set(_lib.RF_CTX_ROWS + _lib.GL_CTX_ROWS))
    ctx = {k: np.full(T, np.nan) for k in rows}
    ctx_ok = np.zeros(T, bool)
    sym = {k: np.full((S, T), NONE if k.startswith("micro") else 0, dtype=np.uint8) for k in KEYS[:5]}
    sym.update({k: np.full((S, T), np.nan) for k in KEYS[5:]})
    entry = {}   # per context column: its symbols' encoded rows, annotated against its predecessor

    def features(j):
        d = batch.context_at(j)
        return batch.symbol_features_at(j, cm, d["btc_return"] if d["btc_present"] else None, btc_index=b)

    seen = before = None
    for t in range(T):
        if valid[t]:
            before, seen = seen, t
        if seen is None:
            continue
        if seen not in entry:
            f = features(seen)
            has = ~np.isnan(f["return_pct"])
            pr = np.full(S, None, dtype=object)
            ps = np.zeros(S)
            if before is not None:
                fp = features(before)
                hp = ~np.isnan(fp["return_pct"])
                pr[hp] = fp["micro_regime"][hp]
                ps[hp] = fp["micro_regime_strength"][hp]
            a = annotate_symbols(f["trend_score"], f["above_ema20"], f["above_ema50"], f["relative_strength_vs_btc"],
                                 f["bb_width"], f["atr_pct"], f["return_pct"], prev_regime=pr, prev_strength=ps)
            e = dict(ok=has.astype(np.uint8),
                     micro_regime=np.array([_lib.MICRO_REGIMES.index(x) for x in a["micro_regime"]], np.uint8),
                     micro_transition=np.array([NONE if x is None else _lib.MICRO_TRANSITIONS.index(x)
                                                for x in a["micro_regime_transition"]], np.uint8),
                     above_ema20=f["above_ema20"].astype(np.uint8), above_ema50=f["above_ema50"].astype(np.uint8),
                     rs_vs_btc=f["relative_strength_vs_btc"], atr_pct=f["atr_pct"], bb_width=f["bb_width"])
            for k in ("micro_regime", "micro_transition"):
                e[k][~has] = NONE
            for k in ("above_ema20", "above_ema50"):
                e[k][~has] = 0
            for k in KEYS[5:]:
                e[k] = np.where(has, e[k], np.nan)
            entry[seen] = e
        d = batch.context_at(seen)
        ctx_ok[t] = True
        ctx["regime_is_transitioning"][t] = float(d["regime_is_transitioning"])
        ctx["market_stress_score"][t] = d["market_stress_score"]
        ctx["market_regime"][t] = _lib.MARKET_REGIMES.index(d["market_regime"])
        ctx["long_regime_score"][t] = d["long_regime_score"]
        for k in KEYS:
            sym[k][:, t] = entry[seen][k]
    host = dict(ctx={k: dev(v) for k, v in ctx.items()}, ok=dev(ctx_ok), sym={k: dev(v) for k, v in sym.items()})
    return px, ind, snap, host


def _equal(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float64:
            assert torch.equal(torch.isnan(x), torch.isnan(y)), k
            x, y = x.nan_to_num(nan=0.0), y.nan_to_num(nan=0.0)
        assert torch.equal(x, y), k


def test_snapshot_tensors_equal_the_host_loop(joined):
    _, _, snap, host = joined
    assert torch.equal(snap.ok, host["ok"])
    rows = tuple(host["ctx"])
    _equal(dict(zip(rows, snap.ctx(rows))), host["ctx"])
    _equal(snap.sym(KEYS), host["sym"])


def test_range_fade_entry_over_the_snapshot(joined):
    px, ind, snap, host = joined
    args = (px["open"], px["high"], px["low"], px["close"], px["volume"], ind["rsi"], ind["bb_upper"], ind["bb_mid"],
            ind["bb_lower"])
    got = signals.range_fade_entry(*args, snap.ctx(_lib.RF_CTX_ROWS), snap.ok, sym=snap.sym(signals.RF_SYM_KEYS))
    want = signals.range_fade_entry(*args, torch.stack([host["ctx"][k] for k in _lib.RF_CTX_ROWS]), host["ok"],
                                    sym={k: host["sym"][k] for k in signals.RF_SYM_KEYS})
    _equal(got, want)
    # the fixture's contexts are mostly RANGE and its symbols take all five micro regimes: the replay stops at the
    # symbol gates on some candles and goes past them on others
    seen = set(torch.unique(got["status"]).tolist())
    assert len(seen) >= 3 and max(seen) >= signals.RF_NO_SYMBOL


def test_grid_ladder_entry_over_the_snapshot(joined):
    px, ind, snap, host = joined
    args = (px["close"], ind["bb_upper"], ind["bb_mid"], ind["bb_lower"])
    got = signals.grid_ladder_entry(*args, snap.ctx(_lib.GL_CTX_ROWS), snap.ok, sym=snap.sym(signals.GL_SYM_KEYS))
    want = signals.grid_ladder_entry(*args, torch.stack([host["ctx"][k] for k in _lib.GL_CTX_ROWS]), host["ok"],
                                     sym={k: host["sym"][k] for k in signals.GL_SYM_KEYS})
    _equal(got, want)
    assert len(torch.unique(got["status"])) >= 3
