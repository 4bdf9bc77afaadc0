"""GPU: bq_grid_ladder_replay (bq_ladder.hip) and its Python layers against
what the real LadderDeployer.signal() did (tests/golden/ladder_gates.npz) and,
at the kernel's tile and 64-slot edges, against the numpy restatement that
fixture pins (tests/ladder_ref.py); signals.grid_only_policy against the
recorded GridOnlyPolicy.resolve table. Codes exact, values bit for bit."""

import numpy as np
import pytest
import torch

from tests import ladder_cases as lc
from tests.ladder_cases import pg, ref

pytestmark = pytest.mark.gpu

W = ref.TILE   # the kernel's tile width


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, pad=7):
    """[S, T] on a row pitch of T + pad."""
    S, T = a.shape
    buf = torch.full((S, T + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = dv(a)
    return buf[:, :T]


def ctx_of(p):
    return dv(np.stack([p["market_regime"].astype(np.float64), np.asarray(p["long_regime_score"], np.float64)]))


def replay(p, *, pad=0, columns=ref.VALUES, bands=None, alias=False, **kw):
    """signals.grid_ladder_entry on numpy inputs; returns replay()'s layout.
    alias: pass the frame's own tensors as `bands`."""
    from binquant_amd import signals

    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    put = (lambda a: pitched(a, pad)) if pad else dv
    close, frame = put(p["close"]), [put(p[k]) for k in lc.BB]
    if alias:
        bands = tuple(frame)
    elif bands is not None:
        bands = tuple(put(b) for b in bands)
    sym = {k: dv(v) for k, v in p["sym"].items()} if p.get("sym") is not None else None
    out = signals.grid_ladder_entry(close, *frame, ctx_of(p), dv(p.get("ctx_ok")), dv(p.get("policy_ok")), bands=bands,
                                    sym=sym, columns=columns, **kw)
    torch.cuda.synchronize()
    assert set(out) == {"status", *columns}
    assert out["status"].dtype == torch.uint8 and all(out[k].dtype == torch.float64 for k in columns)
    assert all(v.shape == p["close"].shape for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(got, want, what, names=ref.VALUES):
    lc.assert_codes_equal(got, want, what)
    lc.assert_values_equal(got, want, what, names)


@pytest.mark.parametrize("recording", lc.RECORDINGS)
def test_fixture_equals_the_real_method(cuda, recording):
    """Row pitch T and T + 7, all columns; and status only."""
    p, want = lc.panel(), lc.recorded(recording)
    rows = dict(first_t=p["first_t"], lens=p["lens"])
    for pad in (0, 7):
        check(replay(p, pad=pad, bands=lc.bands_of(recording), **rows), want, f"{recording}, pad {pad}")
    bare = replay(p, bands=lc.bands_of(recording), columns=(), **rows)
    assert set(bare) == {"status"}
    lc.assert_codes_equal(bare, want, f"{recording}, status only")
    some = replay(p, bands=lc.bands_of(recording), columns=("breakout_high", "bb_change_pct"), **rows)
    check(some, want, f"{recording}, two columns", ("breakout_high", "bb_change_pct"))


@pytest.mark.parametrize("T", [1, 7, 8, 9, 63, 64, 65, W - 1, W, W + 1, W + 63, W + 64])
@pytest.mark.parametrize("S", [1, 3])
def test_step_edges_vs_restatement(cuda, S, T):
    """One and two tiles, a last tile of 1 / 63 / 64 candles; first_t all 0 and
    cycling over 5 / 63 / 64 / 0 with lens = T - 2 on the last row; n = 1, 8
    and the 64-slot halo's limit; the context as [2, 1] and [2, T]; sym as [S],
    [S, T] and None; ld > T."""
    first, lens = lc.edge_rows(S, T)
    for i, (ctx_T, sym) in enumerate(((T, "cell"), (1, "row"), (T, "none"), (1, "cell"))):
        p = lc.edge_panel(S, T, seed=9000 + 17 * T + 5 * S + i, ctx_T=ctx_T, sym=sym)
        for n in (1, 8, 64):
            for f in (None, first):
                want = lc.ref_replay(p, first_t=f, lens=lens, n=n)
                check(replay(p, pad=5, first_t=f, lens=lens, n=n), want, f"{S}x{T} n={n} ctx_T={ctx_T} sym={sym}")
                if sym == "none":
                    assert np.isin(want["status"], (ref.NO_FRAME, ref.POLICY, ref.NO_CONTEXT, ref.NOT_RANGE,
                                                    ref.MICRO_REGIME)).all()


def test_edge_panel_reaches_every_code(cuda):
    """What the edge panels are for: at the two-tile shape every code occurs, and windows reach across the tile edge."""
    S, T = 3, W + 64
    p = lc.edge_panel(S, T, seed=4242)
    want = lc.ref_replay(p)
    seen = np.bincount(want["status"].ravel(), minlength=len(ref.REASONS))
    assert (np.delete(seen, ref.NO_FRAME) > 0).all(), seen
    passing = (want["status"] == ref.EMIT) | (want["status"] > ref.BB_EXPANDING)
    assert passing[:, W:W + 7].any() and passing[:, 64:71].any()
    check(replay(p), want, "two tiles")


def test_thresholds_vs_restatement(cuda):
    """Every parameter away from its default."""
    S, T = 3, 300
    p = lc.edge_panel(S, T, seed=77)
    par = dict(n=5, max_change_pct=8.0, min_width_pct=2.5, max_width_pct=6.0, min_buffer_pct=1.0, max_buffer_pct=2.0,
               atr_multiplier=2.0, min_long_score=0.4)
    want = lc.ref_replay(p, **par)
    assert (want["status"] != lc.ref_replay(p)["status"]).any()
    check(replay(p, **par), want, "thresholds")


def test_from_t_replays_the_newest_candle_alone(cuda):
    p = lc.panel()
    S, T = p["close"].shape
    rows = dict(first_t=p["first_t"], lens=p["lens"])
    full = replay(p, **rows)
    last = replay(p, from_t=np.full(S, T - 1), **rows)
    assert (last["status"][:, :-1] == ref.NO_FRAME).all()
    for k in ref.VALUES:
        assert np.isnan(last[k][:, :-1]).all(), k
    for k in ("status",) + ref.VALUES:
        assert lc.same_bits(last[k][:, -1], full[k][:, -1]).all(), k
    check(last, lc.ref_replay(p, from_t=np.full(S, T - 1), **rows), "from_t = T - 1")
    mixed = np.array([(0, 64, W - 1, W, T - 1, T)[s % 6] for s in range(S)])
    check(replay(p, from_t=mixed, **rows), lc.ref_replay(p, from_t=mixed, **rows), "from_t per row")


def test_aliased_bands_equal_no_bands(cuda):
    p = lc.panel()
    rows = dict(first_t=p["first_t"], lens=p["lens"])
    want = lc.recorded("plain")
    for pad in (0, 7):
        check(replay(p, pad=pad, alias=True, **rows), want, f"aliased, pad {pad}")
    copies = tuple(p[k].copy() for k in lc.BB)   # equal values in other buffers: the two-read path
    check(replay(p, bands=copies, **rows), want, "copied bands")


def test_agrees_with_bb_width_stable(cuda):
    """Where the method reached _bb_stable, bb_change_pct and the verdict are signals.bb_width_stable's."""
    from binquant_amd import signals

    p = lc.panel()
    rows = dict(first_t=dv(p["first_t"]), lens=dv(p["lens"]))
    for n in (8, 3):
        got = replay(p, first_t=p["first_t"], lens=p["lens"], n=n)
        bb = signals.bb_width_stable(*(dv(p[k]) for k in lc.BB), n=n, **rows)
        stable, change = bb["stable"].cpu().numpy(), bb["change_pct"].cpu().numpy()
        walked = (got["status"] == ref.EMIT) | (got["status"] >= ref.BB_EXPANDING)
        assert walked.sum() > 5000
        assert lc.same_bits(got["bb_change_pct"][walked], change[walked]).all()
        assert ((got["status"] != ref.BB_EXPANDING)[walked] == stable[walked]).all()
        assert np.isnan(got["bb_change_pct"][~walked]).all()


def test_grid_only_policy_equals_the_real_method(cuda):
    from binquant_amd import signals

    fx, c = lc.fixture(), lc.policy_cases()
    allow, reason, points = signals.grid_only_policy(dv(c["context_ok"]), dv(c["market_regime"]), dv(c["previous"]),
                                                     dv(c["latest"]))
    torch.cuda.synchronize()
    assert allow.dtype == torch.bool and reason.dtype == torch.uint8 and points.dtype == torch.float64
    assert allow.shape == reason.shape == points.shape == c["previous"].shape
    assert np.array_equal(allow.cpu().numpy(), fx["policy_allow"])
    assert np.array_equal(reason.cpu().numpy(), fx["policy_reason"])
    assert lc.same_bits(points.cpu().numpy(), fx["policy_points"]).all()


def test_policy_feeds_the_entry(cuda):
    """grid_only_policy's `allow` as grid_ladder_entry's policy_ok, per candle time."""
    from binquant_amd import signals

    p = dict(lc.panel())
    T = p["close"].shape[1]
    rng = np.random.default_rng(5)
    prev, lat = rng.uniform(-1, 1, T), rng.uniform(-1, 1, T)
    lat[::7] = prev[::7]
    allow, _, _ = signals.grid_only_policy(dv(p["ctx_ok"]), dv(p["market_regime"]), dv(prev), dv(lat))
    p["policy_ok"] = ref.grid_only_policy(p["ctx_ok"], p["market_regime"], prev, lat)[0]
    assert np.array_equal(allow.cpu().numpy(), p["policy_ok"])
    want = lc.ref_replay(p, first_t=p["first_t"], lens=p["lens"])
    assert (want["status"] == ref.POLICY).any() and (want["status"] == ref.EMIT).any()
    check(replay(p, first_t=p["first_t"], lens=p["lens"]), want, "policy from the fused program")
