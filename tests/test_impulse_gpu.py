"""The impulse-rider and ladder-stability entry gates on the device
(signals.impulse_rider_features / signals.bb_width_stable, bq_impulse.hip):
against the REAL reference's outputs (tests/golden/impulse_gates.npz) and,
at tile and shape edges, against the numpy restatement that fixture pins
(tests/impulse_ref.py). Status exact, values bit for bit, NaN exactly where
the status is not 0."""

import numpy as np
import pytest
import torch

from tests import impulse_cases as ic
from tests.impulse_cases import pg, ref

pytestmark = pytest.mark.gpu


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(values, status):
    return {k: v.cpu().numpy() for k, v in values.items()}, status.cpu().numpy()


def device_gate(p, b_ts, b_close, rows=slice(None), **kw):
    from binquant_amd import signals

    for k in ("first_t", "lens"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    return host(*signals.impulse_rider_features(
        *(dv(p[k][rows]) for k in ("open", "high", "low", "close", "atr", "open_time")), dv(b_ts), dv(b_close), **kw))


def check_vs_ref(p, b_ts, b_close, what, **kw):
    want_v, want_s = ref.impulse_rider(*(p[k] for k in ("open", "high", "low", "close", "atr", "open_time")),
                                       b_ts, b_close, **kw)
    got_v, got_s = device_gate(p, b_ts, b_close, **kw)
    ic.assert_gate_equal(got_v, got_s, want_v, want_s, what)
    return want_s


@pytest.fixture(scope="module")
def panel_runs(cuda):
    """Every recorded run of the fixture panel, one launch each."""
    fx, p = ic.fixture(), ic.panel()
    out = {}
    for name, (symbols, b, thresholds) in ic.runs().items():
        rows = np.array(list(symbols))
        out[name] = (rows, *device_gate(p, p[f"bench_{b}_ts"], p[f"bench_{b}_close"], rows, first_t=p["first_t"][rows],
                                        entry_factor=float(fx["entry_factor"]), **thresholds))
    return out


@pytest.mark.parametrize("name", sorted(ic.runs()))
def test_fixture_panel(panel_runs, name):
    """Default thresholds (a_*) and the wide-open ones (inf_*, g<i>_*: the
    arithmetic at every candle that carries values)."""
    fx = ic.fixture()
    rows, values, status = panel_runs[name]
    pos = fx["positions"][rows]
    take = lambda a: np.take_along_axis(a, pos, axis=1)   # noqa: E731
    want = {k: fx[f"{name}_values"][rows][:, :, i] for i, k in enumerate(fx["keys"])}
    ic.assert_gate_equal({k: take(v) for k, v in values.items()}, take(status), want, fx[f"{name}_status"][rows], name)
    for v in values.values():   # every candle, not only the sampled ones
        assert (np.isnan(v) == (status != 0)).all()


def test_reference_test_frames(cuda):
    """The reference's 20-row frame confirms with entry limit 108.9; its four
    mutations give their four reasons; the hand-built benchmark frames."""
    from binquant_amd import signals

    fx = ic.fixture()
    got = {}
    for i, name in enumerate(str(n) for n in fx["frame_names"]):
        nb = int(fx["frame_nb"][i])
        p = {k: fx[f"frame_{k}"][i:i + 1] for k in ("open", "high", "low", "close", "atr", "open_time")}
        values, status = device_gate(p, fx["frame_bench_ts"][i, :nb], fx["frame_bench_close"][i, :nb])
        assert status[0, -1] == fx["frame_status"][i], name
        assert ic.same_bits(np.array([values[k][0, -1] for k in ref.IR_KEYS]), fx["frame_values"][i]).all(), name
        got[name] = (signals.IR_REASONS[int(status[0, -1])], values)
        assert (status[0, :19] == signals.IR_SHORT_HISTORY).all()
    assert got["reference_frame"][0] == "relative_strength_impulse_confirmed"
    assert got["reference_frame"][1]["entry_limit_price"][0, -1] == pytest.approx(108.9)
    for reason in ("impulse_did_not_cross_threshold", "btc_return_too_high",
                   "confirmation_did_not_hold_trigger_close", "atr_pct_too_high"):
        assert got[f"mutation_{reason}"][0] == reason


def _tile():
    from binquant_amd import engine

    return engine.IMPULSE_TILE


def _t_edges():
    tile = 1024   # engine.IMPULSE_TILE (asserted in the test: collection must not need the library)
    return [1, 6, 19, 20, 26, tile - 1, tile, tile + 1, tile + 6, tile + 7, 2 * tile + 5]


@pytest.mark.parametrize("T", _t_edges())
@pytest.mark.parametrize("S", [1, 3, 70])
def test_tile_and_shape_edges(cuda, S, T):
    """Impulses whose trigger / confirmation pairs and t - 6 anchors straddle
    tile boundaries; first_t mixed per row; ragged lens (0 and < 20 among
    them)."""
    assert _tile() == 1024
    p, b_ts, b_close = ic.injected_panel(S, T, seed=1000 * S + T, tile=_tile())
    g = np.random.default_rng(S * 7 + T)
    first = np.where(g.random(S) < 0.5, 0, g.integers(0, max(T - 5, 1), S))
    lens = g.integers(0, T + 1, S)
    lens[0] = T
    if S > 2:
        lens[1], lens[2] = 0, min(T, 13)
    st = check_vs_ref(p, b_ts, b_close, f"{S}x{T}")
    check_vs_ref(p, b_ts, b_close, f"{S}x{T} first_t/lens", first_t=first, lens=lens)
    if S == 70 and T == 2 * 1024 + 5:
        assert (st == 0).sum() >= 50 and len(np.unique(st)) >= 10
        conf = set(np.argwhere(st == 0)[:, 1].tolist())   # confirmations across the tile boundary
        assert len(conf & set(range(1022, 1032))) >= 4 and len(conf & set(range(2046, 2053))) >= 2


def test_padded_row_pitch(cuda):
    """ld = T + 192 views (the padded enrich outputs) in, contiguous out."""
    from binquant_amd import signals

    S, T = 5, 1100
    p, b_ts, b_close = ic.injected_panel(S, T, seed=5)
    want_v, want_s = ref.impulse_rider(*(p[k] for k in ("open", "high", "low", "close", "atr", "open_time")),
                                       b_ts, b_close)

    def padded(a):
        buf = torch.full((S, T + 192), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :T] = dv(a)
        return buf[:, :T]

    cols = [padded(p[k]) for k in ("open", "high", "low", "close", "atr")]
    assert cols[0].stride(0) == T + 192
    got_v, got_s = host(*signals.impulse_rider_features(*cols, dv(p["open_time"]), dv(b_ts), dv(b_close)))
    ic.assert_gate_equal(got_v, got_s, want_v, want_s, "padded")
    cols[4] = dv(p["atr"])   # the ATR column on its own pitch
    got_v, got_s = host(*signals.impulse_rider_features(*cols, dv(p["open_time"]), dv(b_ts), dv(b_close)))
    ic.assert_gate_equal(got_v, got_s, want_v, want_s, "padded, atr contiguous")
    bands = [padded(p[k]) for k in ("high", "close", "low")]
    res = signals.bb_width_stable(*bands)
    ws, wc = ref.bb_stable(p["high"], p["close"], p["low"])
    np.testing.assert_array_equal(res["stable"].cpu().numpy(), ws)
    assert ic.same_bits(res["change_pct"].cpu().numpy(), wc).all()


def _bench_shapes():
    T = 300
    grid = ic.T0 + ic.STEP * np.arange(T + 40, dtype=np.int64)
    g = np.random.default_rng(99)
    close = 60000.0 * np.exp(np.cumsum(g.normal(0.0, 0.001, T + 40)))
    holes = np.ones(T, bool)
    holes[[57, 140, 141]] = False
    irregular = np.sort(np.r_[grid[:T][g.random(T) < 0.7], grid[:T][::9] + 123_456, grid[5:60] + 60_000])
    dup = np.sort(np.r_[grid[:T], grid[50:T:17], grid[100]])
    return T, {
        "nb0": (grid[:0], close[:0]), "nb4": (grid[20:24], close[20:24]), "nb5": (grid[20:25], close[20:25]),
        "longer": (grid, close), "shorter": (grid[40:170], close[40:170]),
        "half_step": (grid[:T] + ic.STEP // 2, close[:T]),
        "three_holes": (grid[:T][holes], close[:T][holes]),
        "irregular": (irregular, close[:len(irregular)]),
        "duplicates": (dup, close[:len(dup)]),
    }


@pytest.mark.parametrize("shape", sorted(_bench_shapes()[1]))
def test_benchmark_shapes(cuda, shape):
    """Both lookup paths (the guessed row on a regular grid, the search
    otherwise) give impulse_ref's answers."""
    T, shapes = _bench_shapes()
    b_ts, b_close = shapes[shape]
    p, _, _ = ic.injected_panel(6, T, seed=17)
    st = check_vs_ref(p, b_ts, b_close, shape, **ref.WIDE_OPEN | {"min_impulse": 0.0})
    if shape in ("nb0", "nb4", "half_step"):
        assert not (st == 0).any() and (st[:, 19:] <= 4).all()
    elif shape == "nb5":   # one trigger time (candle 24) sits at position 4
        assert (st[:, 25] > 4).any() and (np.delete(st, 25, axis=1)[:, 19:] <= 4).all()
    else:
        assert (st == 0).sum() >= 20, shape


def test_descending_benchmark_is_rejected(cuda):
    from binquant_amd import signals

    p, b_ts, b_close = ic.injected_panel(2, 40, seed=3)
    args = [dv(p[k]) for k in ("open", "high", "low", "close", "atr", "open_time")]
    with pytest.raises(ValueError, match="ascending"):
        signals.impulse_rider_features(*args, dv(b_ts[::-1]), dv(b_close))


def test_null_value_columns(cuda):
    """Only the status, or any single value column, gives the full call's bits."""
    from binquant_amd import signals

    p, b_ts, b_close = ic.injected_panel(9, 1100, seed=23)
    args = [dv(p[k]) for k in ("open", "high", "low", "close", "atr", "open_time")] + [dv(b_ts), dv(b_close)]
    full_v, full_s = signals.impulse_rider_features(*args)
    assert tuple(full_v) == signals.IR_KEYS and int((full_s == 0).sum()) >= 10
    none_v, none_s = signals.impulse_rider_features(*args, columns=())
    assert none_v == {} and torch.equal(none_s, full_s)
    for k in signals.IR_KEYS:
        one_v, one_s = signals.impulse_rider_features(*args, columns=(k,))
        assert list(one_v) == [k] and torch.equal(one_s, full_s)
        assert torch.equal(one_v[k].view(torch.int64), full_v[k].view(torch.int64)), k


@pytest.mark.parametrize("n,max_change", [(8, 20.0), (3, 5.0)])
def test_bb_width_stable_fixture(cuda, n, max_change):
    from binquant_amd import signals

    fx = ic.fixture()
    res = signals.bb_width_stable(dv(fx["bb_upper"]), dv(fx["bb_mid"]), dv(fx["bb_lower"]), n, max_change,
                                  first_t=dv(fx["bb_first_t"]))
    np.testing.assert_array_equal(res["stable"].cpu().numpy(), fx[f"bb_stable_{n}"])
    assert ic.same_bits(res["change_pct"].cpu().numpy(), fx[f"bb_change_{n}"]).all()


def _bands(S, T, seed):
    g = np.random.default_rng(seed)
    mid = 10.0 ** g.uniform(-1, 3, (S, 1)) * np.exp(np.cumsum(g.normal(0, 0.004, (S, T)), axis=1))
    half = mid * 0.02 * np.exp(np.cumsum(g.normal(0, 0.08, (S, T)), axis=1) * 0.5 + g.normal(0, 0.05, (S, T)))
    up, lw = mid + half, mid - half
    for b in range(0, T, 97):   # constant closes (upper == lower), mid <= 0, a NaN in the window
        j = b + 40
        if j + 3 < T:
            up[:, j:j + 3] = lw[:, j:j + 3]
        if j + 30 < T:
            mid[::2, j + 28] = -mid[::2, j + 28]
            mid[1::2, j + 29] = 0.0
        if j + 50 < T:
            up[::3, j + 50] = np.nan
            mid[1::3, j + 51] = np.nan
    return up, mid, lw


@pytest.mark.parametrize("T", _t_edges())
@pytest.mark.parametrize("n", [1, 8, 64])
def test_bb_width_stable_edges(cuda, n, T):
    from binquant_amd import signals

    S = 7
    up, mid, lw = _bands(S, T, seed=31 * n + T)
    g = np.random.default_rng(n + T)
    first = np.where(g.random(S) < 0.5, 0, g.integers(0, max(T - 5, 1), S))
    lens = g.integers(0, T + 1, S)
    lens[0] = T
    for kw in ({}, dict(first_t=first, lens=lens)):
        ws, wc = ref.bb_stable(up, mid, lw, n, 20.0, **kw)
        res = signals.bb_width_stable(dv(up), dv(mid), dv(lw), n, 20.0,
                                      **{k: dv(np.asarray(v, np.int64)) for k, v in kw.items()})
        np.testing.assert_array_equal(res["stable"].cpu().numpy(), ws)
        assert ic.same_bits(res["change_pct"].cpu().numpy(), wc).all()
    if T == 2 * 1024 + 5 and n == 8:   # the inputs hold both outcomes and early returns
        ws, wc = ref.bb_stable(up, mid, lw, n, 20.0)
        assert ws.sum() > 1000 and (~ws & ~np.isnan(wc)).sum() > 1000 and np.isnan(wc[:, 200:]).sum() > 100


def _cohort_inputs(S, T, seed):
    from binquant_amd.synth import numpy_panel

    p5 = numpy_panel(S, T, seed0=seed, edges=True)
    p15, b_ts, b_close = ic.injected_panel(S, T, seed=seed + 1, nan_rate=0.0)
    vol = numpy_panel(S, T, seed0=seed + 2, edges=True)["volume"]
    ins = [dv(p5[k]) for k in ("open", "high", "low", "close", "volume")]
    ins += [dv(p15[k]) for k in ("open", "high", "low", "close")] + [dv(vol)]
    ins += [dv(p15["open_time"]), dv(b_ts), dv(b_close)]
    return ins


def _same(a, b):
    if a.dtype.is_floating_point:
        return torch.equal(torch.nan_to_num(a, nan=-12345.0), torch.nan_to_num(b, nan=-12345.0))
    return torch.equal(a, b)


def test_cohort_gates(cuda):
    """gates=True adds impulse.* / ladder.* equal to direct calls on e15.*;
    every other key is bit-equal to gates=False, whose key set is unchanged;
    captured as a graph and replayed twice it equals eager."""
    import functools

    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline

    S, T = 64, 400
    a, b = _cohort_inputs(S, T, 41), _cohort_inputs(S, T, 43)
    plain = process_cohort(*b)
    gated = process_cohort(*b, gates=True)
    new = [f"impulse.{k}" for k in signals.IR_KEYS] + ["impulse.status", "ladder.stable", "ladder.change_pct"]
    assert not any(k.startswith(("impulse.", "ladder.")) for k in plain)
    assert [k for k in gated if k not in plain] == new and [k for k in gated if k in plain] == list(plain)
    n = int(plain["h1.bins"].max())
    for k in plain:
        x, y = gated[k], plain[k]
        if k.startswith("h1.") and x.dim() == 2:   # bins past a row's count are unwritten
            x, y = x[:, :n], y[:, :n]
        assert _same(x, y), k
    o15, h15, l15, c15, ts15, bts, bc = b[5], b[6], b[7], b[8], b[10], b[11], b[12]
    values, status = signals.impulse_rider_features(o15, h15, l15, c15, gated["e15.ATR"], ts15, bts, bc)
    assert torch.equal(gated["impulse.status"], status) and int((status == 0).sum()) >= 20
    for k, v in values.items():
        assert _same(gated[f"impulse.{k}"], v), k
    ladder = signals.bb_width_stable(gated["e15.bb_upper"], gated["e15.bb_mid"], gated["e15.bb_lower"])
    assert torch.equal(gated["ladder.stable"], ladder["stable"]) and int(ladder["stable"].sum()) > 100
    assert _same(gated["ladder.change_pct"], ladder["change_pct"])
    graph = CapturedPipeline(functools.partial(process_cohort, gates=True), *a)
    for _ in range(2):
        rep = graph(*b)
        torch.cuda.synchronize()
        assert list(rep) == list(gated)
        for k in gated:
            x, y = rep[k], gated[k]
            if k.startswith("h1.") and x.dim() == 2:
                x, y = x[:, :n], y[:, :n]
            assert _same(x, y), f"graph {k}"
