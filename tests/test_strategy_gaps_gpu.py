"""Rows with missing candles through the three strategy pipelines and the a20
helpers, against the REAL reference (tests/golden/strategy_gaps.npz, written by
tests/golden/make_golden_strategy_gaps.py; the rows and their gaps:
tests/golden/strategy_gaps_panel_gen.py):

  a17 ActivityBurstPump.compute_indicators    strategies/activity_burst_pump.py:51-158
  a18 LiquidationSweepPump.compute_pump_score strategies/liquidation_sweep_pump.py:195-269
  a19 FailedSpikeFade.detect                  strategies/failed_spike_fade.py:258-544
  a20 MeanReversionFade._rsi / _trend_score, RangeBbRsiMeanReversion._compute_adx / _compute_zscore

17 rows x 200 candles at every candle and 4 rows x 1100 candles at 960..1099
(the 1024-candle tile edge). Each panel runs whole, one call per pipeline and
mode — gap rows and clean rows share the launches — and every (pipeline,
mode, case) is one test id, e.g. fsf-panel_fused-candle_run.

Bars (tests/test_inf_fixture_gpu.py, tests/test_panel_fixtures_gpu.py,
tests/test_signals_gpu.py): floats by tests.util.assert_close at rtol 1e-9,
scale = the row's largest finite recorded magnitude of the column, NaN
positions and infinities equal; flags, labels and suppressed labels equal in
every mode; the five std columns and their descendants in panel mode through
tests/spike_std.check with its default cap; the calibrated thresholds at
rtol 1e-12; zscore by assert_close_or_exact (max_cases 8 in panel mode, 0 in
exact mode). The two clean rows run alone give the bits they have in the
panel, in every mode."""

import numpy as np
import pytest
import torch

from oracle import indicators_ref
from tests import spike_std
from tests import strategy_gaps as sg
from tests.util import assert_close, assert_close_or_exact

pytestmark = pytest.mark.gpu
gen = sg.gen

LSP_MODES = FSF_MODES = ("exact", "panel_fused", "panel_staged")
ABP_MODES = ("fused", "staged")
A20_MODES = ("rsi_exact", "rsi_panel", "adx_exact", "adx_panel", "zscore_exact", "zscore_panel", "trend")
_SWITCH = {"lsp": "_PUMP_FUSED", "fsf": "_SPIKE_FUSED", "abp": "_BURST_FUSED"}
_results: dict = {}


def _dev(tag, rows=None):
    P = sg.panels()[tag]
    sel = slice(None) if rows is None else np.asarray(rows)
    return {f: torch.from_numpy(np.ascontiguousarray(P[f][sel])).cuda() for f in gen.FIELDS}


def _run(pipe, mode, tag, rows=None):
    """One call of a pipeline in a mode on the rows of a panel (all: cached)."""
    from binquant_amd import signals, strategies

    key = (pipe, mode, tag)
    if rows is None and key in _results:
        return _results[key]
    d = _dev(tag, rows)
    if pipe == "a20":
        name, _, m = mode.partition("_")
        if name == "rsi":
            out = signals.wilder_rsi(d["close"], exact=m == "exact")
        elif name == "adx":
            out = signals.adx(d["high"], d["low"], d["close"], exact=m == "exact")
        elif name == "zscore":
            out = signals.zscore(d["close"], exact=m == "exact")
        else:
            out = signals.trend_score(d["close"])
        out = {name: out.cpu().numpy()}
    else:
        staged = mode in ("panel_staged", "staged")
        if staged:
            setattr(strategies, _SWITCH[pipe], False)
        try:
            if pipe == "lsp":
                btc = torch.from_numpy(sg.bench_aligned(tag)).cuda()
                out = strategies.pump_score_features(d["open"], d["high"], d["low"], d["close"], d["volume"], btc,
                                                     exact=mode == "exact")
            elif pipe == "fsf":
                out = strategies.failed_spike_features(d["open"], d["high"], d["low"], d["close"], d["volume"],
                                                       d["quote_asset_volume"], exact=mode == "exact")
            else:   # even rows (counted through both panels) carry quote_asset_volume, odd rows do not
                n = d["close"].shape[0]
                idx = np.arange(n) if rows is None else np.asarray(rows)
                quote = np.array([gen.has_quote(sg.TAGS[tag][3] + int(i)) for i in idx])
                out = {}
                for q in (True, False):
                    if not (quote == q).any():
                        continue
                    sel = torch.from_numpy(np.flatnonzero(quote == q)).cuda()
                    c = {f: v.index_select(0, sel).contiguous() for f, v in d.items()}
                    part = strategies.activity_burst_features(c["open"], c["high"], c["low"], c["close"], c["volume"],
                                                              c["quote_asset_volume"] if q else None)
                    for k, v in part.items():
                        full = out.setdefault(k, torch.empty((n,) + v.shape[1:], dtype=v.dtype, device=v.device))
                        full[sel] = v
        finally:
            if staged:
                setattr(strategies, _SWITCH[pipe], True)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    if rows is None:
        _results[key] = out
    return out


def _check_row(prefix, out, tag, i, skip=None):
    """Row i of a pipeline's columns against the recorded ones (the rule of
    test_inf_fixture_gpu._check); skip: {column: mask} already explained by
    tests/spike_std.check."""
    z = sg.load()
    lo = sg.TAGS[tag][2]
    keys = sg.columns(prefix)
    assert set(keys) <= set(out), sorted(set(keys) - set(out))
    for k in keys:
        w = z[f"{tag}__{prefix}__{k}"][i]
        g = (out[k] if out[k].ndim == 1 else out[k][i])[lo:]   # [T]: one benchmark series for every row
        name = f"{prefix}.{k}"
        if skip and k in skip:
            g = np.where(skip[k], w.astype(g.dtype), g)
        if g.dtype == bool:
            assert w.dtype == np.uint8, name
            bad = np.flatnonzero(g != w.astype(bool))
            assert bad.size == 0, f"{name}: {bad.size} flags differ, first at candle {lo + int(bad[0])}"
            continue
        assert w.dtype == np.float64, name
        assert_close(g, w, name, rtol=1e-9, scale=sg.row_scale(w))


def _std_skip(mode, tag):
    """tests/spike_std.check on the whole panel, once per mode (its cap counts
    the panel's cells, as in test_panel_fixtures_gpu.test_failed_spike_panel)."""
    key = ("std", mode, tag)
    if key not in _results:
        z = sg.load()
        P = sg.panels()[tag]
        T, lo = sg.TAGS[tag][1], sg.TAGS[tag][2]
        out = _run("fsf", mode, tag)
        S = out["body_size_pct"].shape[0]
        cols = [k for k in set(spike_std.STD_COLS) | set(spike_std.DESC) | {"price_ma", "volume_ma",
                                                                            "body_size_pct_ma_10"}
                if f"{tag}__fsf__{k}" in z]   # detect() returns no volume_std column
        _results[key] = spike_std.check(
            {k: out[k][:, lo:] for k in cols}, {k: z[f"{tag}__fsf__{k}"] for k in cols},
            {"close": P["close"], "volume": P["volume"], "body_size_pct": out["body_size_pct"]},
            positions=np.broadcast_to(np.arange(lo, T), (S, T - lo)))
    return _results[key]


def _fsf(mode, tag, i):
    z = sg.load()
    out = dict(_run("fsf", mode, tag))
    cal = np.array([out.pop("volume_cluster_min_ratio").ravel()[i], out.pop("price_break_base_threshold").ravel()[i]])
    np.testing.assert_allclose(cal, z[f"{tag}__fsf_calibrated"][i], rtol=1e-12)
    skip = None
    if mode != "exact":   # the base pass's window stds: pandas, or the exact window std where pandas drifted
        skip = {k: m[i] for k, m in _std_skip(mode, tag).items()}
    _check_row("fsf", out, tag, i, skip=skip)


def _a20(mode, tag, i):
    z = sg.load()
    P = sg.panels()[tag]
    name = mode.split("_")[0]
    col = "trend_score" if name == "trend" else name
    pos = z[f"{tag}__a20_positions"][i]
    pos = pos[pos >= 0]
    w = z[f"{tag}__a20__{col}"][i][: len(pos)]
    g = _run("a20", mode, tag)[name][i]
    if name != "zscore":
        assert_close(g[pos], w, f"a20.{col}", rtol=1e-9, scale=sg.row_scale(w))
        return
    np.testing.assert_array_equal(np.isnan(g[pos]), np.isnan(w), err_msg="a20.zscore: NaN pattern")
    full_g, full_w = np.full(g.shape, np.nan), np.full(g.shape, np.nan)
    full_g[pos], full_w[pos] = g[pos], w
    assert_close_or_exact(full_g, full_w, P["close"][i], 20, indicators_ref.exact_zscore, "a20.zscore",
                          max_cases=0 if mode == "zscore_exact" else 8)


_MODES = [(p, m) for p, ms in (("lsp", LSP_MODES), ("fsf", FSF_MODES), ("abp", ABP_MODES), ("a20", A20_MODES))
          for m in ms]
_PARAMS = [(p, m, tag, i, case) for p, m in _MODES for tag, i, case in sg.CASES]


@pytest.mark.parametrize("pipe,mode,tag,i,case", _PARAMS, ids=[f"{p}-{m}-{c}" for p, m, _, _, c in _PARAMS])
def test_gap_rows(cuda, pipe, mode, tag, i, case):
    if pipe == "fsf":
        _fsf(mode, tag, i)
    elif pipe == "a20":
        _a20(mode, tag, i)
    else:
        _check_row(pipe, _run(pipe, mode, tag), tag, i)


@pytest.mark.parametrize("pipe,mode", _MODES, ids=[f"{p}-{m}" for p, m in _MODES])
def test_clean_rows_alone_keep_their_bits(cuda, pipe, mode):
    rows = [gen.SHORT_CASES.index(c) for c in gen.CLEAN]
    both = _run(pipe, mode, "short")
    alone = _run(pipe, mode, "short", rows=rows)
    assert list(both) == list(alone)
    for k in both:
        want = both[k] if both[k].ndim == 1 and both[k].shape[0] != len(gen.SHORT_CASES) else both[k][rows]
        np.testing.assert_array_equal(alone[k], want, err_msg=f"{pipe}.{k}")
