"""Batched live-market-context over a [symbols x candles] panel.

Replaces, for every timestamp of the panel at once, the per-message loop of
LiveMarketContextAccumulator.refresh_context_for_timestamp
(market_regime/live_market_context_accumulator.py:72-84): the reference
recomputes _compute_symbol_features for every fresh symbol on every message
(O(S^2 * 400) per 15-minute period). Here:

  1. bq_market_features — per-symbol features at every t (device);
  2. bq_breadth_partial — per-t counts/sums over this rank's symbols (device,
     deterministic order);
  3. all_reduce(sum) of the [T x 10] partials over the symbol shards (RCCL
     over xGMI; the only collective of the whole hot path);
  4. scalar scoring + market-regime annotation over T (host, numpy).

BTC is replicated on every rank (one extra symbol), so relative strength and
the BTC regime score need no communication.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib, engine
from .regime import ContextBatch, annotate_market, annotate_symbols, score_contexts


def seen_columns(valid, timestamps, carry: bool = True, times=None, seeded: bool = False):
    """(at, prev) int64 [T_out] of MarketContextBatch.snapshot, O(T) on the
    host: at[t] the context column candle t sees (-1: none) and prev[t] the
    latest valid column before it (-1: none; -2: the seed, when seeded).
    carry: the latest valid context at or before the candle (the provider's
    latest_market_context), else only the candle's own. times: None (the
    frame is on the contexts' grid) or int64 [T_out] candle close times: the
    latest valid context with timestamp <= time (carry=False: == time)."""
    valid = np.asarray(valid, dtype=bool)
    Tc = len(valid)
    cols = np.arange(Tc, dtype=np.int64)
    last_valid = np.maximum.accumulate(np.where(valid, cols, -1)) if Tc else cols
    before = np.concatenate([[-1], last_valid[:-1]]) if Tc else cols   # the latest valid column before j
    if times is None:
        at = last_valid if carry else np.where(valid, cols, -1)
    else:
        ts = np.asarray(timestamps, dtype=np.int64)
        if Tc > 1 and not (np.diff(ts) > 0).all():
            raise ValueError("snapshot: times= needs ascending context timestamps")
        times = np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times)
        if times.ndim != 1 or times.dtype != np.int64:
            raise ValueError("times: expected a 1-D int64 array of candle close times")
        if not Tc:
            at = np.full(len(times), -1, dtype=np.int64)
        else:
            pos = np.searchsorted(ts, times, side="right") - 1
            safe = np.maximum(pos, 0)
            if carry:
                at = np.where(pos >= 0, last_valid[safe], -1)
            else:
                at = np.where((pos >= 0) & (ts[safe] == times) & valid[safe], safe, -1)
    at = np.asarray(at, dtype=np.int64)
    seen = at >= 0
    prev = np.where(seen, before[np.maximum(at, 0)], -1) if Tc else np.full(len(at), -1, dtype=np.int64)
    if seeded:
        prev = np.where(seen & (prev < 0), -2, prev)
    return at, np.asarray(prev, dtype=np.int64)


@dataclass
class MarketContextBatch:
    contexts: ContextBatch
    features: dict[str, torch.Tensor]   # this rank's [S, T] feature columns
    partial: torch.Tensor               # reduced [T, 10] partials (device)
    rank: torch.Tensor | None = None    # fresh build: [S, T] int32 column of each candle in `features`
    compact_close: torch.Tensor | None = None   # fresh build: the packed close `features` were computed from

    def context_at(self, i: int) -> dict | None:
        return self.contexts.context_at(i)

    def symbol_features_at(self, i: int, close: torch.Tensor, btc_return_t: float | None,
                           btc_index: int | None = None) -> dict[str, np.ndarray]:
        """Per-symbol feature row at timestamp index i (this rank's symbols),
        with relative strength and the micro-regime annotation. After a fused
        build (keep_features=False) only the last timestamp is held. After a
        fresh build (``rank`` set) each symbol's row is gathered at
        rank[:, i]; symbols not fresh at i, or on their first candle, get NaN
        features."""
        T = close.shape[1]
        j = i % T if i < 0 else i
        fcols = next(iter(self.features.values())).shape[1]
        if self.rank is not None:
            k = self.rank[:, j].long()
            have = k >= 1
            idx = k.clamp(min=0)[:, None]
            f = {}
            for name, v in self.features.items():
                row = v.gather(1, idx)[:, 0].double()
                f[name] = torch.where(have, row, torch.full_like(row, float("nan"))).cpu().numpy()
        else:
            if fcols == 1 and T > 1:
                if j != T - 1:
                    raise ValueError("fused context build: only the last timestamp's features are kept")
                j_f = 0
            else:
                j_f = j
            f = {k: v[:, j_f].double().cpu().numpy() for k, v in self.features.items()}
        c = close[:, j].cpu().numpy()
        ret = f["return_pct"]
        rs = np.zeros_like(ret) if btc_return_t is None else ret - btc_return_t
        if btc_index is not None:
            rs[btc_index] = 0.0
        out = dict(f)
        out.update(close=c, above_ema20=c > f["ema20"], above_ema50=c > f["ema50"], relative_strength_vs_btc=rs)
        out.update(annotate_symbols(f["trend_score"], out["above_ema20"], out["above_ema50"], rs,
                                    f["bb_width"], f["atr_pct"], ret))
        return out

    def snapshot(self, close: torch.Tensor, *, btc_index: int | None = None, carry: bool = True, times=None,
                 seed=None, columns=engine.REGIME_PANEL_COLUMNS) -> "PanelSnapshot":
        """What every candle of a panel saw of these contexts, on the device:
        the context's fields and each symbol's symbol_features entry with its
        micro regime and transition (engine.symbol_regime_panel), ready for the
        signals.*_entry panel entries. close: the panel's [S, T] close the
        build was given (this rank's symbols). btc_index: BTC's row, if the
        shard holds it. carry=True: a candle sees the latest valid context at
        or before it (KlinesProvider.latest_market_context,
        consumers/klines_provider.py:181-199); carry=False: only its own
        (accumulator.get_context(ts)). times: int64 [T_out] candle close times
        of a frame on another grid (the 5m frame against 15m contexts): a
        candle then sees the latest valid context with timestamp <= its time
        (carry=False: the one with that very timestamp). A context's
        predecessor is the latest valid one before it (_get_previous_context,
        live_market_context_accumulator.py:86-93); the first valid context has
        none unless `seed` is given: (int8 [S] micro-regime codes, negative
        None; float64 [S] strengths), the symbols' entries in the
        previous_context the build was seeded with. The host part is O(T)
        numpy over contexts.valid / contexts.timestamp; rows are independent,
        so a symbol shard needs nothing beyond its replicated BTC row."""
        valid = np.asarray(self.contexts.valid, dtype=bool)
        Tc = len(valid)
        fcols = next(iter(self.features.values())).shape[1]
        if fcols != Tc:
            raise ValueError("snapshot: a fused context build (keep_features=False) keeps no feature columns")
        if self.rank is not None and self.compact_close is None:
            raise ValueError("snapshot: a fresh build needs compact_close, the packed close of its features")
        at, prev = seen_columns(valid, self.contexts.timestamp, carry=carry, times=times, seeded=seed is not None)
        f = self.contexts.fields
        dev = close.device
        btc = torch.from_numpy(np.where(f["btc_present"], f["btc_return"], np.nan).astype(np.float64)).to(dev)
        sym = engine.symbol_regime_panel(
            self.features, close if self.rank is None else self.compact_close, rank=self.rank, at=at, prev=prev,
            btc_return=btc, btc_row=btc_index, seed=seed, columns=columns)
        return PanelSnapshot(contexts=self.contexts, at=at, columns=sym, device=dev)


_CTX_CODED = {"market_regime", "regime_is_transitioning", "confidence"}


@dataclass
class PanelSnapshot:
    """MarketContextBatch.snapshot's result: per candle of the frame, the
    context it saw (`at`: its column in `contexts`, -1 for none) and, per
    symbol, that context's symbol_features entry (`columns`,
    engine.symbol_regime_panel's tensors [S, T_out])."""

    contexts: ContextBatch
    at: np.ndarray
    columns: dict[str, torch.Tensor]
    device: torch.device

    def _gathered(self, values: np.ndarray, none) -> np.ndarray:
        seen = self.at >= 0
        out = np.full(len(self.at), none, dtype=values.dtype)
        out[seen] = values[self.at[seen]]
        return out

    @property
    def ok(self) -> torch.Tensor:
        """bool [T_out]: a context is seen (the entries' ctx_ok)."""
        return torch.from_numpy(self.at >= 0).to(self.device)

    def ctx(self, rows) -> torch.Tensor:
        """float64 [len(rows), T_out] on the device: the seen context's fields,
        NaN where `ok` is false. rows: any of _lib.PT_CTX_ROWS / MR_CTX_ROWS /
        RF_CTX_ROWS / GL_CTX_ROWS and ContextBatch's numeric fields;
        market_regime is the index into _lib.MARKET_REGIMES,
        regime_is_transitioning 0 / 1, confidence 1.0
        (live_market_context_accumulator.py:213)."""
        f = self.contexts.fields
        out = np.empty((len(rows), len(self.at)), dtype=np.float64)
        for i, name in enumerate(rows):
            if name == "confidence":
                v = np.ones(len(self.contexts.valid))
            elif name == "market_regime":
                v = np.array([_lib.MARKET_REGIMES.index(r) for r in f[name]], dtype=np.float64)
            elif name in f and np.asarray(f[name]).dtype.kind in "fiub":
                v = np.asarray(f[name], dtype=np.float64)
            else:
                known = sorted(_CTX_CODED | {k for k, a in f.items() if np.asarray(a).dtype.kind in "fiub"})
                raise ValueError(f"ctx: unknown row {name!r} (known: {known})")
            out[i] = self._gathered(v, np.nan)
        return torch.from_numpy(out).to(self.device)

    def sym(self, keys, none: str = "uint8") -> dict[str, torch.Tensor]:
        """{key: [S, T_out]} for signals.*_entry(sym=...) and the *_routing /
        *_allows helpers. none="uint8": ok uint8 and micro_regime /
        micro_transition uint8 with _lib.MR_NONE for None (the *_entry
        convention); none="int8": ok bool and the two codes int8, negative for
        None (the helpers' convention)."""
        if none not in ("uint8", "int8"):
            raise ValueError(f"sym: none is 'uint8' (_lib.MR_NONE) or 'int8' (negative), got {none!r}")
        missing = [k for k in keys if k not in self.columns]
        if missing:
            raise ValueError(f"sym: {missing} not among the snapshot's columns {tuple(self.columns)}")
        out = {k: self.columns[k] for k in keys}
        if none == "int8":
            for k in keys:
                if k in ("micro_regime", "micro_transition"):
                    x = out[k]
                    out[k] = torch.where(x == _lib.MR_NONE, -1, x.to(torch.int16)).to(torch.int8)
                elif k == "ok":
                    out[k] = out[k].bool()
        return out

    @property
    def timestamp(self) -> torch.Tensor:
        """int64 [T_out]: the seen context's timestamp (ms), -1 where none."""
        return torch.from_numpy(self._gathered(np.asarray(self.contexts.timestamp, dtype=np.int64), -1)).to(self.device)

    @property
    def regime_stable_since(self) -> torch.Tensor:
        """int64 [T_out]: the seen context's regime_stable_since (ms),
        negative for None (signals.long_autotrade_allows, bb_extreme_routing)."""
        ss = self.contexts.fields["regime_stable_since"]
        v = np.array([-1 if x is None else int(x) for x in ss], dtype=np.int64)
        return torch.from_numpy(self._gathered(v, -1)).to(self.device)


def shard_bounds(n_symbols: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous symbol block of `rank` (S/world per GPU)."""
    base, extra = divmod(n_symbols, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


TRACKED_COLUMN = 9   # PARTIAL_COLUMNS[9]: symbols tracked by the shard


def _all_reduce_sum(buf: torch.Tensor, group) -> None:
    """all_reduce(sum) of buf in place: RCCL over xGMI, or through the host
    when the group is gloo (the CPU rehearsal of the RCCL path)."""
    if buf.is_cuda and dist.get_backend(group) == "gloo":
        host = buf.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        buf.copy_(host)
    else:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)


def reduce_partials(part: torch.Tensor, n_local: int, group=None, force: bool = False,
                    tracked_per_timestamp: bool = False):
    """ONE all_reduce(sum) of the [T, 10] partials over the symbol shards (RCCL
    over xGMI on GPUs, gloo on CPU). The shard's tracked-symbol
    count rides in the spare column 9 of every row, so the admission gate's
    total (live_market_context_accumulator.py:96-102) needs no second
    collective. Returns (reduced partials, total tracked symbols); on one
    rank the partials are returned with column 9 = n_local.

    force=True runs the collective whenever a process group is initialised,
    even at world size 1 (the one-GPU RCCL check, tests/test_rccl_gpu.py).

    tracked_per_timestamp=True (the fresh build): column 9 already holds the
    shard's tracked count at every t (bq_breadth_partial_fresh) and is left as
    written; n_local is not used and the second result is the reduced
    per-timestamp tracked count, an int64 array [T]."""
    collective = dist.is_available() and dist.is_initialized() and (force or dist.get_world_size(group) > 1)
    if tracked_per_timestamp:
        if part.shape[0] and collective:
            _all_reduce_sum(part, group)
        return part, part[:, TRACKED_COLUMN].cpu().numpy().astype(np.int64)
    part[:, TRACKED_COLUMN] = float(n_local)
    if collective:
        # no timestamps (T == 0, the same on every rank): the count alone travels,
        # so every rank still agrees on the admission gate's total
        buf = part if part.shape[0] else torch.full((1, part.shape[1]), float(n_local), dtype=part.dtype,
                                                    device=part.device)
        _all_reduce_sum(buf, group)
        return part, int(buf[0, TRACKED_COLUMN].item())
    return part, int(n_local)


def contexts_from_partials(partial: np.ndarray, btc_return: np.ndarray, btc_trend: np.ndarray,
                           total_tracked, timestamps=None, previous_context: dict | None = None) -> ContextBatch:
    """Host scoring of reduced partials; btc_* are the benchmark's feature rows
    (NaN where it has no features). total_tracked: an int, or a length-T
    array of per-timestamp tracked counts (score_contexts)."""
    btc_valid = ~np.isnan(btc_return)
    batch = score_contexts(partial, np.nan_to_num(btc_return), np.nan_to_num(btc_trend), btc_valid,
                           total_tracked=total_tracked, timestamps=timestamps)
    return annotate_market(batch, previous_context)


def _scored(part, btc_ret, btc_trend, total_tracked, timestamps, previous_context, feats,
            rank=None, compact_close=None) -> MarketContextBatch:
    """The tail of both builds: host scoring of the reduced partials."""
    batch = contexts_from_partials(part.cpu().numpy(), btc_ret, btc_trend, total_tracked=total_tracked,
                                   timestamps=timestamps, previous_context=previous_context)
    return MarketContextBatch(contexts=batch, features=feats, partial=part, rank=rank, compact_close=compact_close)


def _market_context_batch_fresh(high, low, close, btc_hlc, max_bars, timestamps, total_tracked, group,
                                previous_context) -> MarketContextBatch:
    """market_context_batch(fresh=True): compact, features on the compacted
    panel, gathered partials, one all-reduce (column 9 = tracked at t), scoring."""
    comp = engine.compact_panel(high, low, close)
    feats = engine.market_features(comp.high, comp.low, comp.close, max_bars=max_bars)
    part = engine.breadth_partial_fresh(comp, feats)
    part, tracked = reduce_partials(part, close.shape[0], group, tracked_per_timestamp=True)
    # BTC: the features at its last present candle <= t, stale across a gap
    # (its history as it stands, live_market_context_accumulator.py:105-106)
    bcomp = engine.compact_panel(*btc_hlc)
    bf = engine.market_features(bcomp.high, bcomp.low, bcomp.close, max_bars=max_bars)
    k = np.maximum.accumulate(bcomp.rank[0].cpu().numpy().astype(np.int64)) if close.shape[1] else np.zeros(0, np.int64)
    have = k >= 1   # fewer than 2 candles so far: no features (:248-249)
    kk = np.where(have, k, 0)
    btc_ret = np.where(have, bf["return_pct"][0].cpu().numpy()[kk], np.nan)
    btc_trend = np.where(have, bf["trend_score"][0].cpu().numpy()[kk], np.nan)
    return _scored(part, btc_ret, btc_trend, total_tracked if total_tracked is not None else tracked, timestamps,
                   previous_context, feats, comp.rank, comp.close)


def market_context_batch(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    btc_hlc: tuple[torch.Tensor, torch.Tensor, torch.Tensor],
    max_bars: int = 400,
    timestamps: np.ndarray | None = None,
    total_tracked: int | None = None,
    group=None,
    previous_context: dict | None = None,
    keep_features: bool = True,
    fresh: bool = False,
) -> MarketContextBatch:
    """Contexts at every timestamp of a (possibly sharded) [S, T] panel.

    btc_hlc: the benchmark's (high, low, close) [1, T] rows, replicated.
    total_tracked: symbols tracked across ALL ranks (default: sum of shards).
    keep_features=False: the fused build (engine.context_partials) — the
    feature columns are never written; ``features`` then holds the last
    timestamp's row only ([S, 1] each: symbol_features_at(T - 1) works).
    fresh=True: the panel may hold absent candles (NaN close: late listings,
    halts, delistings, gaps) and gets the reference's store semantics — each
    symbol's history is its present candles (market_state_store.py:84, :28),
    a context sums the symbols present at its timestamp (:49-54), the gate
    uses the symbols listed so far (live_market_context_accumulator.py
    :96-102) and BTC's features are those of its last present candle
    (:105-106). ``features`` are then indexed by ``rank``, not by timestamp
    (symbol_features_at gathers). The fused build is dense-only:
    fresh=True needs keep_features=True.
    """
    if fresh:
        if not keep_features:
            raise ValueError("fresh=True needs keep_features=True: the fused context build is dense-only")
        return _market_context_batch_fresh(high, low, close, btc_hlc, max_bars, timestamps, total_tracked, group,
                                           previous_context)
    if keep_features:
        feats = engine.market_features(high, low, close, max_bars=max_bars)
        part = engine.breadth_partial(close, feats)
    else:
        part, last = engine.context_partials(high, low, close, max_bars=max_bars, last=True)
        feats = {k: v[:, None] for k, v in last.items()}
    part, n_total = reduce_partials(part, close.shape[0], group)
    bh, bl, bc = btc_hlc
    bf = engine.market_features(bh, bl, bc, max_bars=max_bars)
    return _scored(part, bf["return_pct"][0].cpu().numpy(), bf["trend_score"][0].cpu().numpy(),
                   total_tracked if total_tracked is not None else n_total, timestamps, previous_context, feats)
