"""Host restatement of engine.symbol_regime_panel (bq_symbol_regime_panel):
regime.annotate_symbols applied column by column under the at / prev rules of
the reference — candle t reads the symbol_features of context column at[t]
(KlinesProvider.latest_market_context + resolve_symbol_features), and a
symbol's transition there is taken against its entry in context column prev[t]
(RegimeTransitionDetector.annotate_context against
accumulator._get_previous_context), none when it has no entry in it."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

from binquant_amd import _lib
from binquant_amd.market_regime.regime import annotate_symbols

G = Path(__file__).resolve().parent / "golden"
if str(G) not in sys.path:
    sys.path.insert(0, str(G))
import regime_panel_gen as gen   # noqa: E402

NONE = _lib.MR_NONE
_REG = {r: i for i, r in enumerate(_lib.MICRO_REGIMES)}
_TRN = {r: i for i, r in enumerate(_lib.MICRO_TRANSITIONS)}


def fixture():
    return np.load(G / "regime_panel.npz")


def context_columns(exists, carry: bool, seed: bool = False):
    """(at, prev) of a frame on the contexts' own grid: the provider's carry
    (the latest valid context at or before t) or the candle's own context;
    prev = the latest valid column before the seen one (-2: the seed)."""
    exists = np.asarray(exists, bool)
    T = len(exists)
    cols = np.arange(T)
    last = np.maximum.accumulate(np.where(exists, cols, -1))
    before = np.concatenate([[-1], last[:-1]])
    at = last if carry else np.where(exists, cols, -1)
    prev = np.where(at >= 0, before[np.maximum(at, 0)], -1)
    if seed:
        prev = np.where((at >= 0) & (prev < 0), -2, prev)
    return at.astype(np.int64), prev.astype(np.int64)


def annotate_panel(trend, above20, above50, rs, bb_width, atr_pct, return_pct, has, at, prev, seed=None):
    """The panel annotation from per-context-column symbol rows ([S, Tc]; has:
    the symbol has an entry in that context). seed: (int8 codes, negative
    None; strengths) [S]. Returns [S, T_out] arrays in symbol_regime_panel's
    encoding (codes uint8 with NONE; float columns NaN where not ok)."""
    S, Tc = np.asarray(has).shape
    at, prev = np.asarray(at), np.asarray(prev)
    To = len(at)
    labels = np.asarray(_lib.MICRO_REGIMES, dtype=object)
    ok = np.zeros((S, To), dtype=np.uint8)
    reg = np.full((S, To), NONE, dtype=np.uint8)
    trn = np.full((S, To), NONE, dtype=np.uint8)
    st = np.full((S, To), np.nan)
    tst = np.full((S, To), np.nan)
    cache = {}

    def column(j):   # every symbol's regime and strength in context column j, once
        if j not in cache:
            a = annotate_symbols(trend[:, j], above20[:, j], above50[:, j], rs[:, j], bb_width[:, j], atr_pct[:, j],
                                 return_pct[:, j])
            cache[j] = (a["micro_regime"], a["micro_regime_strength"])
        return cache[j]

    for t in range(To):
        j = int(at[t])
        if j < 0:
            continue
        h = np.asarray(has[:, j], bool)
        p = int(prev[t])
        pr = np.full(S, None, dtype=object)
        ps = np.zeros(S)
        if p == -2 and seed is not None:
            codes = np.asarray(seed[0])
            pr[codes >= 0] = labels[codes[codes >= 0]]
            ps = np.asarray(seed[1], np.float64)
        elif p >= 0:
            plab, pst = column(p)
            hp = np.asarray(has[:, p], bool)
            pr[hp] = plab[hp]
            ps = np.where(hp, pst, 0.0)
        a = annotate_symbols(trend[:, j], above20[:, j], above50[:, j], rs[:, j], bb_width[:, j], atr_pct[:, j],
                             return_pct[:, j], prev_regime=pr, prev_strength=ps)
        ok[h, t] = 1
        reg[h, t] = [_REG[x] for x in a["micro_regime"][h]]
        trn[h, t] = [NONE if x is None else _TRN[x] for x in a["micro_regime_transition"][h]]
        st[h, t] = a["micro_regime_strength"][h]
        tst[h, t] = a["micro_regime_transition_strength"][h]
    return dict(ok=ok, micro_regime=reg, micro_transition=trn, micro_regime_strength=st,
                micro_transition_strength=tst)


def regime_panel_ref(feats, close, *, rank=None, at=None, prev=None, btc_return=None, btc_row=None, seed=None):
    """engine.symbol_regime_panel on numpy arrays, every column."""
    close = np.asarray(close, np.float64)
    S, Tc = close.shape
    cols = np.arange(Tc)
    if rank is None:
        k = np.broadcast_to(cols, (S, Tc))
    else:
        k = np.asarray(rank, np.int64)
    has = (k >= 1) & (k < Tc)
    kk = np.where(has, k, 0)
    g = {n: np.where(has, np.take_along_axis(np.asarray(feats[n], np.float64), kk, axis=1), np.nan)
         for n in _lib.FEATURE_COLUMNS}
    cl = np.where(has, np.take_along_axis(close, kk, axis=1), np.nan)
    btc = np.full(Tc, np.nan) if btc_return is None else np.asarray(btc_return, np.float64)
    with np.errstate(invalid="ignore"):
        rs = np.where(np.isnan(btc)[None, :], 0.0, g["return_pct"] - btc[None, :])
        if btc_row is not None:
            rs[btc_row] = 0.0
        a20, a50 = cl > g["ema20"], cl > g["ema50"]
    at = cols if at is None else np.asarray(at)
    prev = np.maximum(at - 1, -1) if prev is None else np.asarray(prev)
    out = annotate_panel(g["trend_score"], a20, a50, rs, g["bb_width"], g["atr_pct"], g["return_pct"], has, at, prev,
                         seed)
    seen = np.maximum(at, 0)
    okb = out["ok"].astype(bool)
    out["above_ema20"] = (a20[:, seen] & okb).astype(np.uint8)
    out["above_ema50"] = (a50[:, seen] & okb).astype(np.uint8)
    for name, src in (("rs_vs_btc", rs), ("trend_score", g["trend_score"]), ("atr_pct", g["atr_pct"]),
                      ("bb_width", g["bb_width"])):
        out[name] = np.where(okb, src[:, seen], np.nan)
    return out


def near_cut_columns(feats, close, rank=None, btc_return=None, btc_row=None):
    """regime_panel_gen.near_cut over every (symbol, context column) with features."""
    r = regime_panel_ref(feats, close, rank=rank, btc_return=btc_return, btc_row=btc_row)
    S, Tc = np.asarray(close).shape
    k = np.broadcast_to(np.arange(Tc), (S, Tc)) if rank is None else np.asarray(rank, np.int64)
    has = (k >= 1) & (k < Tc)
    kk = np.where(has, k, 0)
    take = lambda x: np.take_along_axis(np.asarray(x, np.float64), kk, axis=1)  # noqa: E731
    near = gen.near_cut(r["trend_score"], r["above_ema20"], r["above_ema50"], r["rs_vs_btc"], r["bb_width"],
                        r["atr_pct"], take(feats["return_pct"]), take(close), take(feats["ema20"]),
                        take(feats["ema50"]))
    return near & has
