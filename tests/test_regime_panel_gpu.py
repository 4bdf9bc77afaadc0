"""GPU parity of the per-symbol regime panel — engine.symbol_regime_panel
(bq_symbol_regime_panel) and MarketContextBatch.snapshot — against

* the reference itself: MarketStateStore(30) + LiveMarketContextAccumulator
  fed the panel of tests/golden/regime_panel_gen.py
  (make_golden_regime_panel.py; regime_panel.npz): every symbol's entry in
  every context, with the candle's own context and with the provider's
  carried one — no cell left out;
* scoring.micro_regime (bq_micro_regime) on the kernel's own gathered inputs,
  bit for bit;
* the dense build when every candle is present, bit for bit, and itself on a
  second launch;
* the host restatement tests/regime_panel_ref.py on random sparse panels over
  every tile shape, row pitch and at / prev pattern the kernel branches on."""

import numpy as np
import pytest
import torch

from binquant_amd import _lib, engine
from binquant_amd.market_regime import scoring
from binquant_amd.market_regime.batch import market_context_batch, seen_columns
from tests import regime_panel_ref as ref
from tests.util import assert_close

pytestmark = pytest.mark.gpu
U8, F64 = _lib.REGIME_PANEL_U8, _lib.REGIME_PANEL_F64
NONE = _lib.MR_NONE


def _cuda(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit, NaN payloads included"""
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


# ---- the reference's own contexts ---------------------------------------------------

@pytest.fixture(scope="module")
def golden(cuda):
    fx = ref.fixture()
    _, h, l, c, present = ref.gen.build_panel()
    nan = np.where(present, 1.0, np.nan)
    hd, ld, cd = _cuda(h * nan, l * nan, c * nan)
    b = ref.gen.BTC
    batch = market_context_batch(hd, ld, cd, (hd[b:b + 1], ld[b:b + 1], cd[b:b + 1]), max_bars=int(fx["max_bars"]),
                                 timestamps=fx["timestamps"], fresh=True)
    np.testing.assert_array_equal(batch.contexts.valid, fx["exists"])
    return fx, batch, cd


@pytest.mark.parametrize("carry", [False, True])
def test_snapshot_matches_reference_golden(golden, carry):
    fx, batch, close = golden
    snap = batch.snapshot(close, btc_index=ref.gen.BTC, carry=carry)
    at = np.where(fx["exists"], np.arange(ref.gen.T), -1) if not carry else fx["latest"].astype(np.int64)
    np.testing.assert_array_equal(snap.at, at)
    np.testing.assert_array_equal(snap.ok.cpu().numpy(), at >= 0)
    got = _np(snap.columns)
    seen = at >= 0
    j = at[seen]
    has = np.zeros(fx["has"].shape, dtype=bool)
    has[:, seen] = fx["has"][:, j]
    assert has.sum() == fx["has"][:, j].sum() >= 6000   # every cell of every seen context is compared
    np.testing.assert_array_equal(got["ok"], has.astype(np.uint8))
    for name in ("micro_regime", "micro_transition"):
        want = np.full(has.shape, NONE, dtype=np.uint8)
        want[:, seen] = np.where(fx[name][:, j] < 0, NONE, fx[name][:, j]).astype(np.uint8)
        want[~has] = NONE
        np.testing.assert_array_equal(got[name], want, err_msg=name)
    for name in ("above_ema20", "above_ema50"):
        want = np.zeros(has.shape, dtype=np.uint8)
        want[:, seen] = fx[name][:, j]
        np.testing.assert_array_equal(got[name], want * has, err_msg=name)
    for name in F64:   # the features are held to pandas at 1e-9: not bit-equal
        want = np.full(has.shape, np.nan)
        want[:, seen] = fx[name][:, j]
        want[~has] = np.nan
        assert_close(got[name], want, f"{name} carry={carry}")


def test_bit_equal_with_micro_regime(golden):
    """bq_micro_regime on the kernel's own gathered inputs and the predecessor's
    codes and strengths: all four outputs bit for bit — at a column whose
    predecessor is t - 1, at the first after the gated stretch, at the first
    valid one."""
    fx, batch, close = golden
    snap = batch.snapshot(close, btc_index=ref.gen.BTC, carry=False)
    col = snap.columns
    idx = np.flatnonzero(fx["exists"])
    _, prev = seen_columns(fx["exists"], fx["timestamps"], carry=False)
    after_gap = int(idx[1:][np.diff(idx) > 1][0])
    plain = int(idx[len(idx) // 2])
    assert prev[plain] == plain - 1 and prev[after_gap] < after_gap - 1 and prev[idx[0]] == -1
    for t in (plain, after_gap, int(idx[0])):
        ok = col["ok"][:, t].bool()
        assert int(ok.sum()) >= 40
        k = batch.rank[:, t].long().clamp(min=0)[:, None]
        ret = batch.features["return_pct"].gather(1, k)[:, 0]
        p = int(prev[t])
        pr = ps = None
        if p >= 0:
            code = col["micro_regime"][:, p]
            pr = torch.where(code == NONE, -1, code.to(torch.int16)).to(torch.int8)
            ps = col["micro_regime_strength"][:, p].nan_to_num(nan=0.0)
        want = scoring.micro_regime(col["trend_score"][:, t], col["above_ema20"][:, t], col["above_ema50"][:, t],
                                    col["rs_vs_btc"][:, t], col["bb_width"][:, t], col["atr_pct"][:, t], ret,
                                    prev_regime=pr, prev_strength=ps)
        for mine, theirs in (("micro_regime", "micro_regime"), ("micro_transition", "micro_regime_transition")):
            w = want[theirs]
            w = torch.where(w < 0, NONE, w.to(torch.int16)).to(torch.uint8)
            assert torch.equal(col[mine][:, t][ok], w[ok]), (mine, t)
        for mine, theirs in (("micro_regime_strength", "micro_regime_strength"),
                             ("micro_transition_strength", "micro_regime_transition_strength")):
            assert _same(col[mine][:, t][ok], want[theirs][ok]), (mine, t)
        if p >= 0:
            assert int((col["micro_transition"][:, t] != NONE).sum()) > 0, t


# ---- every candle present: the dense build ----------------------------------------------

def test_dense_build_equals_fresh_build_and_repeats(cuda):
    S, T = 48, 300
    # the fixture's kinds of rows, every candle present: calm walks, six sigma = 0.03 rows, six whose drift flips
    g = np.random.default_rng(4242)
    ret = g.normal(0.0002, 0.006, (S, T))
    ret[10:16] = g.normal(0.0, 0.03, (6, T))
    ret[20:26] = np.where((np.arange(T) // 30) % 2 == 0, 0.004, -0.004) + g.normal(0.0, 0.003, (6, T))
    cl = 100.0 * np.exp(np.cumsum(ret, axis=1))
    op = np.concatenate([cl[:, :1], cl[:, :-1]], axis=1)
    h, l, c = _cuda(np.maximum(op, cl) * (1 + g.uniform(0, 0.003, (S, T))),
                    np.minimum(op, cl) * (1 - g.uniform(0, 0.003, (S, T))), cl)
    btc = (h[:1], l[:1], c[:1])
    dense = market_context_batch(h, l, c, btc, max_bars=60)
    fresh = market_context_batch(h, l, c, btc, max_bars=60, fresh=True)
    assert dense.rank is None and fresh.rank is not None and dense.contexts.valid[1:].all()
    a = dense.snapshot(c, btc_index=0)
    b = fresh.snapshot(c, btc_index=0)
    again = dense.snapshot(c, btc_index=0)
    assert set(a.columns) == set(_lib.REGIME_PANEL_COLUMNS)
    for k in _lib.REGIME_PANEL_COLUMNS:
        assert _same(a.columns[k], b.columns[k]), k
        assert _same(a.columns[k], again.columns[k]), k
    assert int(a.columns["ok"].sum()) == S * (T - 1)
    # the comparison is not over one constant: such rows reach the trends and VOLATILE in the fixture
    assert len(torch.unique(a.columns["micro_regime"])) >= 4
    assert int((a.columns["micro_transition"] != NONE).sum()) > 0


# ---- random panels against the host restatement ---------------------------------------

def _random_columns(S, Tc, seed, pad=0):
    """Feature columns as the kernel streams them (any values do: the pass is
    element-wise), clear of every cut by 1e-6; with pad, as views of
    [S, Tc + pad] buffers."""
    for attempt in range(20):
        g = np.random.default_rng(seed + 1000 * attempt)
        close = 100.0 * np.exp(g.normal(0, 0.2, (S, Tc)))
        off = lambda: g.choice([-1.0, 1.0], (S, Tc)) * g.uniform(0.001, 0.03, (S, Tc))   # noqa: E731  (no close ~ ema)
        f = dict(return_pct=g.normal(0, 0.015, (S, Tc)), ema20=close * (1 + off()), ema50=close * (1 + off()),
                 trend_score=g.normal(0, 0.015, (S, Tc)),
                 atr_pct=g.uniform(0.0, 0.07, (S, Tc)), bb_width=g.uniform(0.0, 0.16, (S, Tc)))
        btc = g.normal(0, 0.01, Tc)
        btc[g.random(Tc) < 0.1] = np.nan
        present = g.random((S, Tc)) < 0.85
        rank = np.where(present, np.cumsum(present, axis=1) - 1, -1).astype(np.int32)
        if not (ref.near_cut_columns(f, close, None, btc, 0).any() or ref.near_cut_columns(f, close, rank, btc, 0).any()):
            break
    else:
        raise AssertionError("no panel clear of the cuts")

    def dev(x):
        if not pad:
            return torch.from_numpy(x).cuda()
        buf = torch.full((S, Tc + pad), float("nan") if x.dtype == np.float64 else -1, dtype=torch.from_numpy(x).dtype,
                         device="cuda")
        buf[:, :Tc] = torch.from_numpy(x).cuda()
        return buf[:, :Tc]

    return f, close, btc, rank, {k: dev(v) for k, v in f.items()}, dev(close), torch.from_numpy(btc).cuda(), dev(rank)


def _check(got, want, what):
    got = _np(got)
    for k in U8:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    for k in F64:   # the same inputs through the same operations
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("S", [1, 5, 37])
def test_random_panels_match_restatement(cuda, S, T):
    f, close, btc, rank, fd, cd, bd, rd = _random_columns(S, T, seed=S * 1000 + T)
    g = np.random.default_rng(T)
    valid = g.random(T) < 0.8
    at, prev = seen_columns(valid, np.arange(T), carry=True)
    for name, rk, rkd in (("dense", None, None), ("fresh", rank, rd)):
        # every context valid: each tile takes the in-order path
        got = engine.symbol_regime_panel(fd, cd, rank=rkd, btc_return=bd, btc_row=0)
        _check(got, ref.regime_panel_ref(f, close, rank=rk, btc_return=btc, btc_row=0), f"{name} in order")
        # 20 % invalid contexts, carried: tiles that gather
        got = engine.symbol_regime_panel(fd, cd, rank=rkd, at=at, prev=prev, btc_return=bd, btc_row=0)
        _check(got, ref.regime_panel_ref(f, close, rank=rk, at=at, prev=prev, btc_return=btc, btc_row=0),
               f"{name} carried")


def test_padded_row_pitch(cuda):
    S, T = 5, 257
    f, close, btc, rank, fd, cd, bd, rd = _random_columns(S, T, seed=77, pad=192)
    assert fd["ema20"].stride(0) == T + 192 and rd.stride(0) == T + 192
    for rk, rkd in ((None, None), (rank, rd)):
        got = engine.symbol_regime_panel(fd, cd, rank=rkd, btc_return=bd)
        _check(got, ref.regime_panel_ref(f, close, rank=rk, btc_return=btc), "padded")


def test_all_invalid_and_far_predecessor(cuda):
    S, T = 5, 700
    f, close, btc, rank, fd, cd, bd, rd = _random_columns(S, T, seed=78)
    none = np.full(T, -1)
    got = _np(engine.symbol_regime_panel(fd, cd, rank=rd, at=none, prev=none, btc_return=bd))
    assert not got["ok"].any() and (got["micro_regime"] == NONE).all() and (got["micro_transition"] == NONE).all()
    assert not got["above_ema20"].any() and all(np.isnan(got[k]).all() for k in F64)
    # no valid context over 100 .. 449: the predecessor of column 450 lies more than one tile back
    valid = np.ones(T, bool)
    valid[100:450] = False
    for carry in (True, False):
        at, prev = seen_columns(valid, np.arange(T), carry=carry)
        assert prev[450] == 99
        got = engine.symbol_regime_panel(fd, cd, rank=rd, at=at, prev=prev, btc_return=bd, btc_row=2)
        _check(got, ref.regime_panel_ref(f, close, rank=rank, at=at, prev=prev, btc_return=btc, btc_row=2),
               f"gap carry={carry}")


def test_times_on_a_finer_grid(cuda):
    S, T = 5, 130
    f, close, btc, rank, fd, cd, bd, rd = _random_columns(S, T, seed=79)
    valid = np.random.default_rng(3).random(T) < 0.7
    ts = 900 * np.arange(1, T + 1, dtype=np.int64)
    times = 300 * np.arange(1, 3 * T + 1, dtype=np.int64)   # 5m closes against 15m contexts
    at, prev = seen_columns(valid, ts, carry=True, times=times)
    assert len(at) == 3 * T and (at >= 0).any() and (at[:2] == -1).all()
    got = engine.symbol_regime_panel(fd, cd, rank=rd, at=at, prev=prev, btc_return=bd)
    assert got["ok"].shape == (S, 3 * T)
    _check(got, ref.regime_panel_ref(f, close, rank=rank, at=at, prev=prev, btc_return=btc), "finer grid")


def test_seed_carries_a_chunked_replay(cuda):
    S, T, cut = 37, 513, 300
    f, close, btc, rank, fd, cd, bd, rd = _random_columns(S, T, seed=80)
    whole = engine.symbol_regime_panel(fd, cd, rank=rd, btc_return=bd, btc_row=0)
    code = whole["micro_regime"][:, cut - 1]
    seed = (torch.where(code == NONE, -1, code.to(torch.int16)).to(torch.int8).contiguous(),
            whole["micro_regime_strength"][:, cut - 1].nan_to_num(nan=0.0).contiguous())
    at = np.arange(cut, T)
    prev = at - 1
    prev[0] = -2
    part = engine.symbol_regime_panel(fd, cd, rank=rd, at=at, prev=prev, btc_return=bd, btc_row=0, seed=seed)
    for k in _lib.REGIME_PANEL_COLUMNS:
        assert _same(part[k], whole[k][:, cut:]), k
    assert int((part["micro_transition"][:, 0] != NONE).sum()) > 0   # the seed was read
    want = ref.regime_panel_ref(f, close, rank=rank, at=at, prev=prev, btc_return=btc, btc_row=0,
                                seed=tuple(x.cpu().numpy() for x in seed))
    _check(part, want, "seeded chunk")
    # without a seed the chunk's first candle has no predecessor
    bare = engine.symbol_regime_panel(fd, cd, rank=rd, at=at, prev=prev, btc_return=bd, btc_row=0)
    assert (bare["micro_transition"][:, 0] == NONE).all()


def test_columns_left_out_are_not_allocated(cuda):
    S, T = 5, 257
    f, close, btc, rank, fd, cd, bd, rd = _random_columns(S, T, seed=81)
    valid = np.random.default_rng(4).random(T) < 0.8
    at, prev = seen_columns(valid, np.arange(T), carry=True)
    for kw in (dict(), dict(at=at, prev=prev)):
        full = engine.symbol_regime_panel(fd, cd, rank=rd, btc_return=bd, **kw)
        for cols in (("ok",), ("ok", "above_ema20", "atr_pct"), ("micro_regime", "bb_width"),
                     ("micro_transition_strength",), ("ok", "micro_regime", "micro_transition", "atr_pct", "bb_width")):
            part = engine.symbol_regime_panel(fd, cd, rank=rd, btc_return=bd, columns=cols, **kw)
            assert tuple(part) == cols
            for k in cols:
                assert _same(part[k], full[k]), (cols, k)
