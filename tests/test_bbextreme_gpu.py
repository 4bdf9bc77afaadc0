"""GPU: bq_bb_extreme_replay (bq_bbextreme.hip) and its Python layers against
what the real methods did (tests/golden/bbextreme_gates.npz) and, at the
kernel's step edges, against the numpy restatement that fixture pins
(tests/bbextreme_ref.py). Codes exact, values bit for bit: the kernel performs
the method's IEEE operations in its order."""

import numpy as np
import pytest
import torch

from tests import bbextreme_cases as bc
from tests.bbextreme_cases import pg, ref

pytestmark = pytest.mark.gpu


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, pad=7):
    """[S, T] on a row pitch of T + pad."""
    S, T = a.shape
    buf = torch.full((S, T + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = dv(a)
    return buf[:, :T]


def replay(p, *, pad=0, columns=ref.VALUES, **kw):
    """signals.bb_extreme_entry on numpy inputs; returns replay()'s layout."""
    from binquant_amd import signals

    put = (lambda a: pitched(a, pad)) if pad else dv
    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    out = signals.bb_extreme_entry(put(p["close"]), *(put(p[k]) for k in bc.BANDS), columns=columns, **kw)
    torch.cuda.synchronize()
    assert set(out) == {"status", *columns}
    assert out["status"].dtype == torch.uint8 and all(out[k].dtype == torch.float64 for k in columns)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("window", bc.WINDOWS)
def test_fixture_is_bit_exact(cuda, window):
    p, want = bc.panel(), bc.recorded(window)
    for pad in (0, 7):
        got = replay(p, pad=pad, first_t=p["first_t"], lens=p["lens"], rsi_window=window)
        bc.assert_codes_equal(got, want, f"kernel, rsi_window {window}, pad {pad}")
        bc.assert_values_bits(got, want, f"kernel, rsi_window {window}, pad {pad}")


FIRSTS = (0, 35, 63, 64)


def edge_rows(S, T):
    first = np.array([FIRSTS[s % 4] for s in range(S)]).clip(0, max(T - 1, 0))
    lens = np.full(S, T)   # rows 0-3 hold the planted NaN / infinite closes, counted from the newest candle
    if S > 4:
        lens[4] = max(T - 2, 1)
    return first, lens


@pytest.mark.parametrize("T", [29, 30, 31, 63, 64, 65, 93, 94, 128, 129])
@pytest.mark.parametrize("S", [1, 4, 5])
def test_step_edges_vs_restatement(cuda, S, T):
    """A full (4 rows) and a partial workgroup of waves; first_t 0 / 35 / 63 /
    64 (at T = 93 / 94 the row starting at 64 has 29 / 30 candles); ld > T."""
    p = bc.edge_panel(S, T, seed=5000 + 11 * T + S)
    for first in (np.zeros(S, np.int64), edge_rows(S, T)[0]):
        lens = edge_rows(S, T)[1]
        want = bc.ref_replay(p, first_t=first, lens=lens)
        got = replay(p, pad=5, first_t=first, lens=lens)
        bc.assert_codes_equal(got, want, f"{S}x{T}")
        bc.assert_values_bits(got, want, f"{S}x{T}")
    if S == 5 and T == 129:   # what the panel is for
        want = bc.ref_replay(p)
        seen = np.bincount(want["status"].ravel(), minlength=7)
        assert (seen[[ref.EMIT, ref.NOT_ENOUGH_DATA, ref.NULLS, ref.NO_RSI, ref.INVALID_BAND, ref.NO_EXTREME]] > 0).all()
        emit = want["status"] == ref.EMIT
        assert (want["direction"][emit] == ref.BUY).any() and (want["direction"][emit] == ref.SELL).any()
        assert want["status"][0, -1] != ref.NULLS and want["status"][1, -1] == ref.NULLS   # a NaN 30 / 29 back
        assert want["status"][2, -1] == ref.NO_RSI and want["status"][3, -1] != ref.NULLS


@pytest.mark.parametrize("params", [
    dict(lookback=2, rsi_window=1), dict(lookback=64), dict(lookback=64, rsi_window=63), dict(rsi_window=1),
    dict(rsi_window=29), dict(rsi_window=30), dict(lookback=1, rsi_window=1), dict(lookback=33, rsi_window=14),
    dict(oversold_rsi=30.0, overbought_rsi=70.0, max_lower_band_position=0.6, min_upper_band_position=0.4),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_parameters_vs_restatement(cuda, params):
    """lookback 2 and 64, rsi_window 1 / 29 / 30 (30 + 1 > lookback: every
    eligible candle is NO_RSI), other thresholds (a NaN span's band_position
    0.5 can emit under them); the planted NaN / infinite closes sit at the
    distances of these parameters."""
    S, T = 5, 200   # at lookback 64 the rows starting at 63 / 64 still have 70 eligible candles
    L, W = params.get("lookback", 30), params.get("rsi_window", 2)
    p = bc.edge_panel(S, T, seed=77 + L + 3 * W, lookback=L, window=min(W, L))
    first = edge_rows(S, T)[0]
    want = bc.ref_replay(p, first_t=first, **params)
    got = replay(p, pad=3, first_t=first, **params)
    bc.assert_codes_equal(got, want, str(params))
    bc.assert_values_bits(got, want, str(params))
    if W + 1 > L:
        reached = want["status"] >= ref.NO_RSI
        assert reached.any() and (want["status"][reached] == ref.NO_RSI).all()
        assert (want["rsi_value"][reached] == 50.0).all()
    elif W <= 2:
        assert (want["status"] == ref.EMIT).any()
    # a NaN exactly lookback - 1 candles back is in the window, one exactly lookback back is not
    if L > 1:
        assert want["status"][1, -1] == ref.NULLS and want["status"][0, -1] != ref.NULLS


def test_newest_candle_only_and_status_alone(cuda):
    """from_t at the newest candle (a cohort message): the one column equals
    the whole replay's; every value column NULL."""
    for T in (64, 65, 94, 129):
        S = 5
        p = bc.edge_panel(S, T, seed=900 + T)
        first, lens = edge_rows(S, T)
        whole = bc.ref_replay(p, first_t=first, lens=lens)
        got = replay(p, first_t=first, lens=lens, from_t=lens - 1)
        for s in range(S):
            n = int(lens[s]) - 1
            assert (got["status"][s, :n] == ref.NO_FRAME).all() and (got["status"][s, n + 1:] == ref.NO_FRAME).all()
            assert got["status"][s, n] == whole["status"][s, n], (T, s)
            for k in ref.VALUES:
                assert bc.same_bits(got[k][s, n], whole[k][s, n]).all(), (T, s, k)
                assert np.isnan(got[k][s, :n]).all()
        alone = replay(p, first_t=first, lens=lens, columns=())
        bc.assert_codes_equal(alone, whole, f"status alone, T {T}")
        one = replay(p, first_t=first, lens=lens, columns=("direction",))
        bc.assert_values_bits(one, whole, f"one column, T {T}", names=("direction",))


@pytest.mark.parametrize("k", [63, 64, 65])
def test_split_replay_equals_whole(cuda, k):
    S, T = 5, 200
    p = bc.edge_panel(S, T, seed=300 + k)
    first = edge_rows(S, T)[0]
    whole = replay(p, first_t=first)
    a = replay(p, first_t=first, lens=np.full(S, k))
    b = replay(p, first_t=first, from_t=np.full(S, k))
    for name in ("status",) + ref.VALUES:
        joined = np.concatenate([a[name][:, :k], b[name][:, k:]], axis=1)
        assert bc.same_bits(joined, whole[name]).all() if name in ref.VALUES else (joined == whole[name]).all(), name
    assert (b["status"][:, :k] == ref.NO_FRAME).all() and (a["status"][:, k:] == ref.NO_FRAME).all()
    bc.assert_codes_equal(whole, bc.ref_replay(p, first_t=first), "5x200")


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    S, T = 3, 40
    p = bc.edge_panel(S, T, seed=1)
    c, up, mid, lo = (dv(p[k]) for k in ("close",) + bc.BANDS)
    engine.bb_extreme_replay(c, up, mid, lo)
    engine.bb_extreme_replay(c, up, mid, lo, rsi_window=40)   # the method's own branch
    for bad in (dict(lookback=0), dict(lookback=65), dict(rsi_window=0), dict(nope=1), dict(oversold_rsi=float("nan")),
                dict(min_upper_band_position=float("inf")), dict(columns=("nope",)), dict(first_t=[0, 1]),
                dict(lens=torch.ones(S))):
        with pytest.raises(ValueError):
            engine.bb_extreme_replay(c, up, mid, lo, **bad)
    for args in ((c.float(), up, mid, lo), (c[0], up, mid, lo), (c, up[:, :5], mid, lo), (c, up, mid.float(), lo),
                 (c, up, mid, lo[:2]), (c.cpu(), up, mid, lo), (c, up, mid, lo.cpu()),
                 (c.t().contiguous().t(), up, mid, lo)):
        with pytest.raises(ValueError):
            engine.bb_extreme_replay(*args)


def test_routing_equals_recorded_table(cuda):
    from binquant_amd import signals

    fx, cs = bc.fixture(), pg.routing_cases()
    assert signals.BBX_ROUTE_REASONS == ref.ROUTE_REASONS == tuple(fx["reasons"])
    col = lambda a: dv(np.asarray(a).reshape(-1, 1))   # noqa: E731  ([N, 1]: one case per row)
    auto, route = signals.bb_extreme_routing(
        col(cs["context_ok"]), col(cs["transitioning"]), col(cs["timestamp"]), col(cs["stable_since"]),
        col(cs["stress"]), col(cs["market_regime"]), col(cs["features_ok"]), col(cs["micro_regime"]),
        col(cs["micro_transition"]), col(cs["strength"]), col(cs["direction"]))
    assert auto.dtype == torch.bool and route.dtype == torch.uint8
    assert auto.shape == route.shape == (len(fx["routing_reason"]), 1)
    assert route.cpu().numpy().ravel().tolist() == fx["routing_reason"].tolist()
    assert auto.cpu().numpy().ravel().tolist() == fx["routing_autotrade"].tolist()
    # the panel's own contexts: [T] context fields against [S, T] features and the replay's direction column
    p = bc.panel()
    ctx_ok = p["market_kind"] != pg.MARKET_KINDS.index("none")
    feats_ok = np.array(pg.IN_SNAPSHOT)[:, None] & ctx_ok[None, :]
    for window in bc.WINDOWS:
        rec = bc.recorded(window)
        direction = replay(p, first_t=p["first_t"], lens=p["lens"], rsi_window=window,
                           columns=("direction",))["direction"]
        auto, route = signals.bb_extreme_routing(
            dv(ctx_ok), dv(p["transitioning"]), dv(p["timestamp"]), dv(p["stable_since"]), dv(p["stress"]),
            dv(p["market_regime"]), dv(feats_ok), dv(p["micro_regime"]), dv(p["micro_transition"]), dv(p["strength"]),
            dv(direction))
        emit = rec["status"] == ref.EMIT
        assert (route.cpu().numpy()[emit] == rec["route"][emit]).all()
        assert (auto.cpu().numpy()[emit] == rec["autotrade"][emit]).all()
