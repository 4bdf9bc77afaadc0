"""a11 on the device for rows with missing (NaN) and zero closes, against the
reference: the recorded values of ContextEvaluator.dynamic_btc_beta_corr on
every prefix (tests/golden/beta_corr_gaps.npz) and the oracle's
beta_corr_prefix, which tests/test_beta_gaps.py pins to them.

The contract (oracle.indicators_ref.beta_corr_prefix): the window at candle t
is the last `window` valid return pairs however far back they lie; NaN while
fewer exist, while the variance is 0 and while the window holds a +-inf
return (a zero close); a candle without a pair repeats the last valid pair's
value. assert_close compares the NaN pattern exactly, so NaN and a computed 0
are told apart wherever the comparison is with beta_corr_prefix."""

import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import frame_ref as fref
from oracle import indicators_ref as ref
from tests.test_beta_gaps import GAP_CASES, W, gap_case
from tests.util import assert_close

NAN = float("nan")
BENCH = ("clean", "nan_tile_edge", "zero_close")


def device_beta_corr(close, btc, window, odd_stride=False):
    from binquant_amd import engine

    S, T = close.shape
    ld = T + 1 if odd_stride else T
    buf = torch.zeros((S, ld), dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.from_numpy(np.array(close)).cuda()   # copies: the shared panels are read-only
    out = engine.beta_corr(buf[:, :T], torch.from_numpy(np.array(btc)).cuda(), window=window)
    return out["beta"].cpu().numpy(), out["corr"].cpu().numpy()


# ---- the reference's own values ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", GAP_CASES)
def test_kernel_matches_reference_golden_with_gaps(cuda, case):
    c, b, want_b, want_c = gap_case(case)
    beta, corr = device_beta_corr(c[None], b, W)
    beta, corr = beta[0], corr[0]
    assert np.isnan(beta[0]) and np.isnan(corr[0])
    assert_close(np.nan_to_num(beta[1:]), want_b[1:], "beta", rtol=1e-9, scale=1.0)
    assert_close(np.nan_to_num(corr[1:]), want_c[1:], "corr", rtol=1e-9, scale=1.0)
    pb, pc = ref.beta_corr_prefix(c, b, W)   # NaN where the reference maps NaN to 0, 0 where it computes 0
    assert_close(beta, pb, "beta vs prefix oracle", rtol=1e-9, scale=1.0)
    assert_close(corr, pc, "corr vs prefix oracle", rtol=1e-9, scale=1.0)


# ---- seeded panels ------------------------------------------------------------
def gap_panel(T, window, group, bench):
    """close [S <= 8, T], btc [T] and the rows' names. Group "edges": gaps at
    the row ends and at the wave kernel's 256-candle tile edges, a gap longer
    than the 128-candle halo, zero closes; group "runs": halts, rows with
    (almost) no pairs, gaps that meet the benchmark's."""
    rng = np.random.default_rng(1000 * T + 10 * window + len(group))
    S = 8
    r = rng.normal(0.0, 0.01, size=(S + 1, T))
    jumps = rng.random((S + 1, T)) < 0.02
    r[jumps] = rng.choice([-0.4, -0.15, 0.14, 0.5], size=int(jumps.sum()))
    p = 50.0 * np.exp(np.cumsum(r, axis=1))
    close, btc = p[:S], p[S].copy()
    edge = [1023, 1024] if T > 1024 else [T // 2, T // 2 + 1]   # the pre-pass's 1024-candle tile edge
    if bench == "nan_tile_edge":
        btc[edge] = NAN
    elif bench == "zero_close":
        btc[300] = 0.0
    if group == "edges":
        names = ["clean", "nan_0", "nan_1", "nan_last", "nan_tile_edges", "gap_150", "zero_mid_tile", "zero_at_1"]
        close[1, 0] = NAN
        close[2, 1] = NAN
        close[3, T - 1] = NAN
        close[4, [255, 256, 257, 511, 512]] = NAN
        close[5, 330:480] = NAN            # the window-th valid pair lies outside the LDS ring
        close[6, 390] = 0.0
        close[7, 1] = 0.0                  # the row reference rx
    else:
        names = ["clean", "halt_with_nan", "all_nan", "few_pairs", "zero_at_0", "meets_benchmark", "every_third",
                 "nan_run_to_end"]
        close[1, 400:480] = close[1, 399]
        close[1, 440] = NAN
        close[2, :] = NAN
        close[3, : T - (window - 1)] = NAN   # window - 2 pairs
        close[4, 0] = 0.0
        close[5, [edge[0], 299, 300, 301]] = NAN
        close[6, 100:400:3] = NAN          # pairs only every third candle: windows reach 3 * window back
        close[7, T - 200:] = NAN           # delisted: the last valid pair's value to the end
    return close, btc, names


@functools.lru_cache(maxsize=None)
def gap_panel_reference(T, window, group, bench):
    close, btc, names = gap_panel(T, window, group, bench)
    want = [ref.beta_corr_prefix(close[s], btc, window) for s in range(close.shape[0])]
    for a in [close, btc] + [v for bc in want for v in bc]:
        a.setflags(write=False)
    return close, btc, names, want


def test_gap_panels_hold_what_they_claim():
    for T in (700, 1337):
        close, btc, names, want = gap_panel_reference(T, 50, "edges", "clean")
        assert not np.isnan(close[0]).any() and np.isnan(close[5]).sum() == 150 > 128
        assert np.isnan(want[5][0][330:481]).sum() == 0 and np.isnan(want[6][0]).sum() == 50 + 51
        assert np.isnan(want[7][0][:52]).all() and not np.isnan(want[7][0][52:]).any()
        close, btc, names, want = gap_panel_reference(T, 50, "runs", "nan_tile_edge")
        assert np.isnan(want[2][0]).all() and np.isnan(want[3][0]).all() and np.isnan(btc).sum() == 2
        assert (want[1][0][452:480] == 0.0).all() and np.isnan(want[1][1][452:480]).all()
        assert (want[7][0][T - 200:] == want[7][0][T - 201]).all() and not np.isnan(want[7][0][T - 201])


@pytest.mark.gpu
@pytest.mark.parametrize("bench", BENCH)
@pytest.mark.parametrize("group", ["edges", "runs"])
@pytest.mark.parametrize("odd_stride", [False, True])
@pytest.mark.parametrize("window", [5, 50, 126])
@pytest.mark.parametrize("T", [700, 1337])
def test_kernel_matches_prefix_oracle_on_gap_panels(cuda, T, window, odd_stride, group, bench):
    """Windows 5 (gaps exceed the window), 50, and 126 (the window nearly
    fills the 128-candle halo); contiguous rows and an odd row stride; gaps in
    the symbol rows together with a clean benchmark, one with NaNs at the
    pre-pass's tile edge and one with a zero close."""
    close, btc, names, want = gap_panel_reference(T, window, group, bench)
    beta, corr = device_beta_corr(close, btc, window, odd_stride)
    for s, name in enumerate(names):
        assert_close(beta[s], want[s][0], f"beta[{name}]", rtol=1e-8, scale=1.0)
        assert_close(corr[s], want[s][1], f"corr[{name}]", rtol=1e-8, scale=1.0)


# ---- every entry point ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bench", ["clean", "nan_tile_edge"])
@pytest.mark.parametrize("group", ["edges", "runs"])
def test_entry_points_agree_on_gap_panels(cuda, group, bench):
    """bq_beta_corr_ws (the engine's, MODE 4), bq_beta_corr (MODE 0) and
    bq_beta_corr_bret with scratch (MODE 3) and without (MODE 2): equal to
    1e-12 where finite, one NaN pattern."""
    from binquant_amd import _lib, engine

    T, w = 1337, 50
    close, btc, names, _ = gap_panel_reference(T, w, group, bench)
    S = close.shape[0]
    c = torch.from_numpy(np.array(close)).cuda()
    b = torch.from_numpy(np.array(btc)).cuda()
    ws = engine.beta_corr(c, b, w)
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    outs = {}
    beta0, corr0 = torch.empty_like(c), torch.empty_like(c)
    _lib.check(lib.bq_beta_corr(vp(c), vp(b), S, T, T, w, vp(beta0), vp(corr0), T, None), "bq_beta_corr")
    outs["bq_beta_corr"] = (beta0, corr0)
    bret = torch.full((T,), NAN, dtype=torch.float64, device="cuda")
    torch.log(b[1:] / b[:-1], out=bret[1:])
    scratch = torch.empty(3 * T, dtype=torch.float64, device="cuda")
    for name, scr in (("bret+scratch", vp(scratch)), ("bret", None)):
        beta, corr = torch.empty_like(c), torch.empty_like(c)
        _lib.check(lib.bq_beta_corr_bret(vp(c), vp(bret), scr, S, T, T, w, vp(beta), vp(corr), T, None),
                   "bq_beta_corr_bret")
        outs[name] = (beta, corr)
    torch.cuda.synchronize()
    wb, wc = ws["beta"].cpu().numpy(), ws["corr"].cpu().numpy()
    for name, (beta, corr) in outs.items():
        assert_close(beta.cpu().numpy(), wb, f"{name} beta", rtol=1e-12, scale=1.0)
        assert_close(corr.cpu().numpy(), wc, f"{name} corr", rtol=1e-12, scale=1.0)


# ---- joined pairs that carry -inf / +inf ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("bench_zero", [False, True])
@pytest.mark.parametrize("window", [50, 20])
def test_joined_pairs_with_zero_closes_match_reference(cuda, window, bench_zero):
    """The frames of test_joined_returns_and_beta_corr_match_reference with
    zero closes: dropna keeps the -inf and +inf returns, so the compacted
    pairs carry them into bq_beta_corr_pairs."""
    from binquant_amd import engine

    M15 = 900_000
    rng = np.random.default_rng(window)
    base = 1_700_000_000_000
    S, T = 6, 700
    bts = base + M15 * np.sort(rng.choice(900, 800, replace=False))
    bclose = 30000 * np.exp(np.cumsum(rng.normal(0, 0.003, bts.size)))
    ts = base + M15 * np.sort(np.stack([rng.choice(900, T, replace=False) for _ in range(S)]), axis=1)
    close = 10 * np.exp(np.cumsum(rng.normal(0, 0.004, (S, T)), axis=1))
    close[0, 300] = 0.0
    close[3, 1] = 0.0      # the row's first pairs
    close[4, 255] = 0.0    # the +inf return opens the second tile
    if bench_zero:
        bclose[420] = 0.0
    lens = np.array([T, 40, 0, 500, T, 2])
    x, y, n = engine.join_returns(torch.from_numpy(ts).cuda(), torch.from_numpy(close).cuda(),
                                  torch.from_numpy(bts).cuda(), torch.from_numpy(bclose).cuda(), lens=lens)
    bc = engine.beta_corr_pairs(x, y, window)
    x, y, n = x.cpu().numpy(), y.cpu().numpy(), n.cpu().numpy()
    beta, corr = bc["beta"].cpu().numpy(), bc["corr"].cpu().numpy()
    infs = 0
    for s in range(S):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = fref.joined_returns(ts[s, : lens[s]], close[s, : lens[s]], bts, bclose)
        k = len(r)
        assert n[s] == k
        infs += int(np.isinf(r.to_numpy()).sum())
        np.testing.assert_array_equal(np.isinf(x[s, :k]), np.isinf(r["alt"].to_numpy()))
        np.testing.assert_array_equal(np.isinf(y[s, :k]), np.isinf(r["btc"].to_numpy()))
        if k:
            wb, wc = fref.beta_corr_series(r, window)
            assert_close(beta[s, :k], wb, f"beta[{s}]", rtol=1e-9, scale=np.nanmax(np.abs(wb)) if k >= window else 1.0)
            assert_close(corr[s, :k], wc, f"corr[{s}]", rtol=1e-9, scale=1.0)
    assert infs >= 4


# ---- clean rows in a launch with gap rows ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("window", [50, 126])
def test_clean_rows_keep_their_bits_next_to_gap_rows(cuda, window):
    T = 1337
    close, btc, names, _ = gap_panel_reference(T, window, "edges", "clean")
    close = close.copy()
    clean = [0, 2, 5]
    rng = np.random.default_rng(window)
    close[clean] = 20.0 * np.exp(np.cumsum(rng.normal(0.0, 0.01, (len(clean), T)), axis=1))
    assert np.isfinite(close[clean]).all() and np.isfinite(btc).all() and (btc > 0).all()
    assert all(not np.isfinite(close[s]).all() or (close[s] == 0).any() for s in range(8) if s not in clean)
    mixed = device_beta_corr(close, btc, window)
    alone = device_beta_corr(close[clean], btc, window)
    for got, want in zip(mixed, alone):
        assert got[clean].tobytes() == want.tobytes()


# ---- the drop-ins -------------------------------------------------------------------------
@pytest.mark.gpu
def test_dropin_scalar_with_gaps(cuda):
    from binquant_amd.indicators import dynamic_btc_beta_corr

    c, b, want_b, want_c = gap_case("gap_alt")
    assert np.isnan(c[-1]) and want_b[-1] != 0.0   # the reference answers with the last valid pair
    beta, corr = dynamic_btc_beta_corr(pd.DataFrame({"close": c}), pd.DataFrame({"close": b}), decimals=None)
    assert beta == pytest.approx(want_b[-1], rel=1e-9, abs=1e-12)
    assert corr == pytest.approx(want_c[-1], rel=1e-9, abs=1e-12)
    c, b, want_b, want_c = gap_case("sparse")
    assert dynamic_btc_beta_corr(pd.DataFrame({"close": c}), pd.DataFrame({"close": b}), decimals=None) == (0.0, 0.0)
