"""GPU: bq_rs_reversal_replay (bq_rsreversal.hip) and its Python layers against
what the real method did (tests/golden/rsreversal_gates.npz) and, at the
kernel's step edges, against the numpy restatement that fixture pins
(tests/rsreversal_ref.py). Codes exact; the floor equal or both NaN, which is
bit equality except for a zero's sign (np.sort and the kernel's key order may
pick either of two equal zeros)."""

import numpy as np
import pytest
import torch

from tests import rsreversal_cases as rc
from tests.rsreversal_cases import ref

pytestmark = pytest.mark.gpu


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, pad=7):
    """[S, T] on a row pitch of T + pad."""
    S, T = a.shape
    buf = torch.full((S, T + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = dv(a)
    return buf[:, :T]


def replay(p, *, pad=0, columns=ref.VALUES, **kw):
    """signals.rs_reversal_entry on numpy inputs; returns replay()'s layout."""
    from binquant_amd import signals

    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    vol = pitched(p["volume"], pad) if pad else dv(p["volume"])
    out = signals.rs_reversal_entry(vol, *(dv(p[k]) for k in rc.CTX), columns=columns, **kw)
    torch.cuda.synchronize()
    assert set(out) == {"status", *columns}
    assert out["status"].dtype == torch.uint8 and all(out[k].dtype == torch.float64 for k in columns)
    assert all(v.shape == p["volume"].shape for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(got, want, what):
    rc.assert_codes_equal(got, want, what)
    rc.assert_values_equal(got, want, what)


def test_fixture_equals_the_real_method(cuda):
    p, want = rc.panel(), rc.recorded()
    for pad in (0, 7):
        got = replay(p, pad=pad, first_t=p["first_t"], lens=p["lens"])
        check(got, want, f"kernel, pad {pad}")


@pytest.mark.parametrize("T", [95, 96, 97, 127, 128, 129, 159, 160, 161, 192, 193])
@pytest.mark.parametrize("S", [1, 4, 5])
def test_step_edges_vs_restatement(cuda, S, T):
    """A full (4 rows) and a partial workgroup of waves; first_t all 0 and
    cycling over 0 / 31 / 63 / 64 (at T = 159 the row starting at 64 has no
    eligible candle, at T = 160 exactly one); a row with lens = T - 2; a NaN
    exactly window - 1 and window candles before the newest; ld > T."""
    p = rc.edge_panel(S, T, seed=7000 + 13 * T + S)
    first, lens = rc.edge_rows(S, T)
    for f in (np.zeros(S, np.int64), first):
        want = rc.ref_replay(p, first_t=f, lens=lens)
        check(replay(p, pad=5, first_t=f, lens=lens), want, f"{S}x{T}")
        if S >= 4 and f is first:
            eligible = (want["status"][3] != ref.NO_FRAME) & (want["status"][3] != ref.SHORT_FRAME)
            assert eligible.sum() == max(int(lens[3]) - 159, 0)
    if S == 5 and T == 193:   # what the panel is for
        want = rc.ref_replay(p)
        seen = np.bincount(want["status"].ravel(), minlength=10)
        assert (np.delete(seen, ref.NO_FRAME) > 0).all(), seen
        w = ref.DEFAULTS["window"]
        assert np.isnan(p["volume"][0, T - 1 - w]) and np.isnan(p["volume"][1, T - w])


@pytest.mark.parametrize("quantile", [0.0, 0.2, 0.5, 0.92, 1.0])
@pytest.mark.parametrize("window", [1, 2, 64, 65, 66, 129, 130, 192])
def test_windows_and_quantiles_vs_restatement(cuda, window, quantile):
    """window 65 / 66: the 128- / 256-slot switch; 129 / 130: the widest
    window whose sorted union serves two steps, and the first that sorts every
    step. With window 1 the floor is
    the candle's own volume, and at quantile 1.0 it is the window's maximum:
    every finite reached cell is DEAD_TAPE (unless its window holds an
    infinity: inf - inf in the lerp, a NaN floor)."""
    S, T = 5, 330   # at window 192 the rows starting at 63 / 64 still have 70 eligible candles
    p = rc.edge_panel(S, T, seed=31 * window + int(100 * quantile), window=window)
    first, lens = rc.edge_rows(S, T)
    want = rc.ref_replay(p, first_t=first, lens=lens, window=window, quantile=quantile)
    check(replay(p, pad=3, first_t=first, lens=lens, window=window, quantile=quantile), want, f"w {window} q {quantile}")
    reached = (want["status"] == ref.EMIT) | (want["status"] == ref.DEAD_TAPE)
    assert reached.sum() >= 100 and (want["status"] == ref.DEAD_TAPE).any()
    if window == 1 or quantile == 1.0:   # where the window's maximum is infinite the lerp is inf - inf: NaN, emitted
        clean = np.array([[t + 1 >= window and not np.isinf(p["volume"][s, t - window + 1:t + 1]).any()
                           for t in range(T)] for s in range(S)])
        finite = reached & np.isfinite(p["volume"]) & clean
        assert (window > 2 or finite.sum() >= 100) and (want["status"][finite] == ref.DEAD_TAPE).all()
    if window > 1:   # a NaN exactly window - 1 candles back is in the newest window, one exactly window back is not
        assert np.isnan(p["volume"][0, T - 1 - window]) and np.isnan(p["volume"][1, T - window])


@pytest.mark.parametrize("case", [
    dict(avg_return_max=0.01, rs_min=-0.1), dict(avg_return_max=-0.05, rs_min=0.2), dict(ctx_T=1),
    dict(ctx_T=1, per_cell=False), dict(per_cell=False), dict(no_flags=True),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_thresholds_and_argument_shapes(cuda, case):
    """Other thresholds; one context for every candle (ctx_T 1) and one per
    candle; features_ok / rs per row and per cell; context_ok / features_ok None."""
    case = dict(case)
    S, T = 5, 200
    shape = {k: case.pop(k) for k in ("ctx_T", "per_cell") if k in case}
    none = case.pop("no_flags", False)
    p = rc.edge_panel(S, T, seed=99, **shape)
    if shape.get("ctx_T") == 1:   # a context that passes, so that the rows' own gates decide
        p.update(context_ok=np.ones(1, bool), market_regime=np.full(1, ref.RANGE, np.int8),
                 average_return=np.full(1, -0.03))
    if not shape.get("per_cell", True):   # one entry per row: a row at the limit (refused) and one without features
        p["rs"][1], p["features_ok"][2] = 0.05, False
    if none:
        p.update(context_ok=None, features_ok=None)
    first, lens = rc.edge_rows(S, T)
    want = rc.ref_replay(p, first_t=first, lens=lens, **case)
    check(replay(p, first_t=first, lens=lens, **case), want, str(case))
    assert ((want["status"] == ref.EMIT).any() and (want["status"] == ref.DEAD_TAPE).any()
            and (want["status"] == ref.RS_INSUFFICIENT).any())


@pytest.mark.parametrize("through", ["none", "all", "steps"])
def test_context_patterns(cuda, through):
    """A context that lets no candle through (codes only, every floor NaN), one
    that lets every candle through, and one that alternates per 64-candle
    step: the skip path and the sort path meet."""
    S, T = 5, 300
    p = rc.edge_panel(S, T, seed=500 + len(through), through=through)
    first, lens = rc.edge_rows(S, T)
    want = rc.ref_replay(p, first_t=first, lens=lens)
    got = replay(p, pad=1, first_t=first, lens=lens)
    check(got, want, through)
    reached = (want["status"] == ref.EMIT) | (want["status"] == ref.DEAD_TAPE)
    if through == "none":
        assert not reached.any() and np.isnan(got["volume_floor"]).all()
    elif through == "all":
        assert (reached == (want["status"] != ref.NO_FRAME) & (want["status"] != ref.SHORT_FRAME)).all()
    else:
        step = (np.arange(T) // 64)[None, :].repeat(S, 0)
        assert not reached[step % 2 == 0].any() and all(reached[step == k].any() for k in (1, 3))


def test_newest_candle_only_and_status_alone(cuda):
    """from_t at the newest candle (a cohort message): the one column equals
    the whole replay's; the value column NULL."""
    for T in (128, 129, 160, 193):
        S = 5
        p = rc.edge_panel(S, T, seed=900 + T, through="all")
        first, lens = rc.edge_rows(S, T)
        whole = rc.ref_replay(p, first_t=first, lens=lens)
        got = replay(p, first_t=first, lens=lens, from_t=lens - 1)
        for s in range(S):
            n = int(lens[s]) - 1
            assert (got["status"][s, :n] == ref.NO_FRAME).all() and (got["status"][s, n + 1:] == ref.NO_FRAME).all()
            assert got["status"][s, n] == whole["status"][s, n], (T, s)
            assert rc.same_value(got["volume_floor"][s, n], whole["volume_floor"][s, n]).all(), (T, s)
            assert np.isnan(got["volume_floor"][s, :n]).all()
        alone = replay(p, first_t=first, lens=lens, columns=())
        rc.assert_codes_equal(alone, whole, f"status alone, T {T}")


@pytest.mark.parametrize("k", [63, 64, 65, 127, 128, 129, 159, 160, 161, 191, 192, 193])
def test_split_replay_equals_whole(cuda, k):
    """lens = k / from_t = k on either side of a 64-candle step edge: at 63 /
    64 / 65 the first half is all short frames, at 127-129 and 191-193 both
    halves hold reached cells (a row ends on a step's last candle, a replay
    starts on a step's first with no floors handed on); 159-161 split inside a
    step, between a sorted step's own floors and the ones it hands on."""
    S, T = 5, 260
    p = rc.edge_panel(S, T, seed=300 + k)
    first = rc.edge_rows(S, T)[0]
    whole = replay(p, first_t=first)
    a = replay(p, first_t=first, lens=np.full(S, k))
    b = replay(p, first_t=first, from_t=np.full(S, k))
    for name in ("status",) + ref.VALUES:
        joined = np.concatenate([a[name][:, :k], b[name][:, k:]], axis=1)
        assert rc.same_value(joined, whole[name]).all(), name
    assert (b["status"][:, :k] == ref.NO_FRAME).all() and (a["status"][:, k:] == ref.NO_FRAME).all()
    want = rc.ref_replay(p, first_t=first)
    check(whole, want, "5x260")
    reached = (want["status"] == ref.EMIT) | (want["status"] == ref.DEAD_TAPE)
    assert reached[:, k:].any() and (k < 127 or reached[:, :k].any())


def test_floor_equals_the_row_quantile(cuda):
    """On NaN-free rows the floor at the newest candle is engine.row_quantile
    of the row's last `window` volumes (bq_select.hip's index and lerp)."""
    from binquant_amd import engine

    S, T, W = 6, 150, 96
    rng = np.random.default_rng(4)
    p = rc.edge_panel(S, T, seed=12, through="all")
    p["volume"] = np.round(rng.lognormal(3.0, 0.7, (S, T)), 1)
    p["volume"][1, 100], p["volume"][2, 60:140] = np.inf, np.inf
    tail = dv(p["volume"][:, T - W:])
    for q in (0.2, 0.37):
        assert q * 100.0 / 100.0 == q
        got = replay(p, quantile=q)
        assert (got["status"][:, -1] != ref.NO_FRAME).all()
        want = engine.row_quantile(tail, q).cpu().numpy()
        assert rc.same_value(got["volume_floor"][:, -1], want).all(), q


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    S, T = 3, 120
    p = rc.edge_panel(S, T, seed=1)
    v, ok, mk, ar, fok, rs = (dv(p[k]) for k in ("volume",) + rc.CTX)
    engine.rs_reversal_replay(v, ok, mk, ar, fok, rs)
    engine.rs_reversal_replay(v, None, mk[:1], ar[:1], None, rs[:, 0].contiguous(), window=192)   # every candle short
    for bad in (dict(window=0), dict(window=193), dict(quantile=1.01), dict(quantile=float("nan")), dict(nope=1),
                dict(rs_min=float("nan")), dict(avg_return_max=float("inf")), dict(columns=("nope",)),
                dict(first_t=[0, 1]), dict(lens=torch.ones(S))):
        with pytest.raises(ValueError):
            engine.rs_reversal_replay(v, ok, mk, ar, fok, rs, **bad)
    for args in ((v.float(), ok, mk, ar, fok, rs), (v[0], ok, mk, ar, fok, rs), (v, ok[:5], mk, ar, fok, rs),
                 (v, ok, mk.long(), ar, fok, rs), (v, ok, mk[:7], ar, fok, rs), (v, ok, mk, ar.float(), fok, rs),
                 (v, ok, mk, ar[:1], fok, rs), (v, ok, mk, ar, fok[:2], rs), (v, ok, mk, ar, fok, rs.float()),
                 (v, ok, mk, ar, fok[:, 0], rs), (v.cpu(), ok, mk, ar, fok, rs), (v, ok, mk.cpu(), ar, fok, rs),
                 (v, ok, mk, ar, fok, rs.cpu()), (v.t().contiguous().t(), ok, mk, ar, fok, rs)):
        with pytest.raises(ValueError):
            engine.rs_reversal_replay(*args)
