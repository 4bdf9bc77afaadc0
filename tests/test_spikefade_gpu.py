"""FailedSpikeFade.signal()'s pending-spike replay on the device
(signals.failed_spike_fade / engine.spike_fade_replay, bq_spikefade.hip):
against what the REAL method did candle by candle (tests/golden/spikefade_gates.npz)
and, at the kernel's step edges, against the numpy restatement that fixture
pins (tests/spikefade_ref.py). Events, detail bits, bars and states: all
exact (every test is a compare and at most one correctly rounded multiply)."""

import functools

import numpy as np
import pytest
import torch

from tests import spikefade_cases as sc
from tests.spikefade_cases import pg, ref

pytestmark = pytest.mark.gpu

STATE_DTYPES = (np.uint8, np.int64, np.float64, np.float64)


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(res):
    return tuple(x.cpu().numpy() for x in res)


def device_state(state):
    return tuple(dv(np.asarray(x, dt)) for x, dt in zip(state, STATE_DTYPES))


def replay(p, state=None, rows=slice(None), masks=True, **kw):
    """engine.spike_fade_replay on numpy inputs; returns (event, detail,
    bars) and, with a state, the state after the call."""
    from binquant_amd import engine

    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    st = device_state(state) if state is not None else None
    m = [dv(p[k][rows]) if masks and p.get(k) is not None else None for k in ("src_market", "fail_market")]
    res = engine.spike_fade_replay(*(dv(p[k][rows]) for k in sc.COLS + ("open_time", "source_ok")), *m, state=st, **kw)
    return host(res), (host(st) if st is not None else None)


def test_kernel_equals_reference_panel(cuda):
    """All rows in one launch; the carry-out state is the recorded
    strategy_states entry after each row's last candle."""
    fx, p = sc.fixture(), sc.panel()
    got, state = replay(sc.fixture_inputs(), state=sc.idle_state(pg.S), first_t=p["first_t"], lens=p["lens"],
                        from_t=p["first_t"], **sc.fixture_params())
    sc.assert_replay_equal(got, (fx["event"], fx["detail"], fx["bars"]), "panel")
    sc.assert_state_equal(state, sc.recorded_state(p["lens"] - 1), "carry-out")
    stateless, _ = replay(sc.fixture_inputs(), first_t=p["first_t"], lens=p["lens"])
    sc.assert_replay_equal(stateless, got, "no state, default parameters, from_t below first_t")


@pytest.mark.parametrize("split", range(5))
def test_resume_from_recorded_state(cuda, split):
    """From the recorded state after candle k - 1 (k: a seeded split point
    per row, 5 per row in all), candles [k, lens) reproduce the recording."""
    fx, p = sc.fixture(), sc.panel()
    g = np.random.default_rng(100 + split)
    k = g.integers(p["first_t"] + 20, p["lens"])
    got, state = replay(sc.fixture_inputs(), state=sc.recorded_state(k - 1), first_t=p["first_t"], lens=p["lens"],
                        from_t=k, **sc.fixture_params())
    cols = np.arange(pg.T)
    tail = (cols >= k[:, None]) & (cols < p["lens"][:, None])
    for name, x, want in zip(("event", "detail", "bars"), got, (fx["event"], fx["detail"], fx["bars"])):
        assert (x[tail] == want[tail]).all(), name
        assert (x[~tail] == (ref.FS_NO_FRAME if name == "event" else 0)).all(), name
    sc.assert_state_equal(state, sc.recorded_state(p["lens"] - 1), f"split {split}")
    assert sc.recorded_state(k - 1)[0].any()   # some rows resume with a spike pending


def test_repeated_message_is_same_candle(cuda):
    """The generator's second message on a source candle: from the recorded
    state the kernel answers SAME_CANDLE and leaves the state as it was."""
    fx, p = sc.fixture(), sc.panel()
    rep = fx["repeats"]
    from_t = np.array(p["lens"])
    state = [np.array(x) for x in sc.idle_state(pg.S)]
    for s, t in rep:
        from_t[s] = t
        for dst, src in zip(state, sc.recorded_state(np.array([t]), [s])):
            dst[s] = src[0]
    lens = np.where(from_t < p["lens"], from_t + 1, p["lens"])
    got, after = replay(sc.fixture_inputs(), state=state, first_t=p["first_t"], lens=lens, from_t=from_t)
    rows = np.unique(rep[:, 0])
    assert (got[0][rows, from_t[rows]] == ref.FS_SAME_CANDLE).all()
    assert (got[1][rows, from_t[rows]] == 0).all() and (got[2][rows, from_t[rows]] == 0).all()
    assert (np.delete(got[0], rows, axis=0) == ref.FS_NO_FRAME).all()
    sc.assert_state_equal(after, state, "a repeat leaves the state")


EDGE_T = (1, 9, 63, 64, 65, 127, 128, 129, 200)
EDGE_S = (1, 4, 5, 9)


@pytest.mark.parametrize("T", EDGE_T)
def test_step_edges_vs_restatement(cuda, T):
    """Every (S, T) of the grid (four waves per workgroup: S = 1, 5 and 9 end
    in a partial workgroup), window_bars 1 / 8 / 32: sources at lane 63 with
    the failure at lane 0 of the next step, the candidate at bars == window
    and the expiry at bars == window + 1 across a step edge, three or more
    set / resolve cycles inside a step, missing highs and whole windows of
    them; then ragged rows (lens < T, from_t mid-step, first_t > 0) with
    carried-in spikes, a NaN st_high among them."""
    from binquant_amd import engine

    seen, bits = np.zeros(6, np.int64), 0
    for S in EDGE_S:
        for W in (1, 8, 32):
            p = sc.edge_panel(S, T, seed=1000 * T + 10 * S + W, window=W)
            want = sc.replay_ref(p, window_bars=W)
            got, state = replay(p, state=sc.idle_state(S), window_bars=W)
            sc.assert_replay_equal(got, want, f"S={S} T={T} W={W}")
            sc.assert_state_equal(state, want[3], f"S={S} T={T} W={W}")
            seen += np.bincount(want[0].ravel(), minlength=256)[:6]
            bits |= int(np.bitwise_or.reduce(want[1].ravel()))
            if S == 9 and T == 200:   # the situations the panel is for, counted on the restatement
                ev, dt, br = want[:3]
                lane = np.arange(T) % sc.WAVE
                assert ((ev[0] == ref.FS_SOURCE_SET) & (lane == 63)).sum() >= 3
                assert ((ev[0] == ref.FS_CANDIDATE) & (lane == 0) & (br[0] == 1)).sum() >= 3
                assert ((ev[1] == ref.FS_CANDIDATE) & (br[1] == W) & (lane == 0)).sum() >= 1
                assert ((ev[1] == ref.FS_CLEARED) & (dt[1] == ref.D_WINDOW_EXPIRED) & (br[1] == W + 1)
                        & (lane == 1)).sum() >= 1
                if W <= 8:
                    sets = (ev[2][:192].reshape(3, 64) == ref.FS_SOURCE_SET).sum(axis=1)
                    assert sets.max() >= 3, sets
                window_all_nan = [np.isnan(p["high"][5, t - b + 1:t + 1]).all() for t, b in zip(*np.nonzero(br[5:6])[1:],
                                                                                                  br[5][br[5] > 0])]
                assert any(window_all_nan) and np.isnan(p["high"][4]).any()
    if T >= 127:
        assert (seen[:5] >= 10).all(), seen
        assert bits == (ref.D_SOURCE | ref.D_MARKET | ref.D_NEW_HIGH | ref.D_WINDOW_EXPIRED | ref.D_EXTENSION), bits
    # ragged rows, a late start and carried-in spikes (found, NaN high, not found)
    S, W = 9, 8
    p = sc.edge_panel(S, T, seed=T, window=W)
    g = np.random.default_rng(T)
    lens = g.integers(0, T + 1, S)
    lens[0] = T
    from_t = np.minimum(g.integers(0, T, S), lens)
    from_t[1] = 0
    from_t[2] = min(T - 1, 70)   # mid-step
    first = np.where(g.random(S) < 0.5, 0, g.integers(0, max(T - 20, 1), S))
    back = np.maximum(from_t - g.integers(0, 12, S), 0)
    rows = np.arange(S)
    state = (np.array([1, 0, 1, 1, 1, 0, 1, 1, 1], np.uint8), p["open_time"][rows, back],
             p["high"][rows, back] * 1.001, p["close"][rows, back])
    state[1][3] -= 1          # an open time no candle has
    state[2][4] = np.nan      # a NaN st_high fails every compare
    kw = dict(first_t=first, lens=lens, from_t=from_t, window_bars=W)
    want2 = sc.replay_ref(p, state=state, **kw)
    got2, st2 = replay(p, state=state, **kw)
    sc.assert_replay_equal(got2, want2, f"T={T} ragged")
    sc.assert_state_equal(st2, want2[3], f"T={T} ragged")
    # a padded row pitch on every input (ld = T + 192), event only
    def padded(a):
        t = dv(a)
        buf = torch.zeros((t.shape[0], T + 192), dtype=t.dtype, device="cuda")
        buf[:, :T] = t
        return buf[:, :T]

    cols = [padded(p[k]) for k in sc.COLS + ("open_time", "source_ok", "src_market", "fail_market")]
    e4, d4, b4 = engine.spike_fade_replay(*cols, detail=False, bars=False, window_bars=W)
    assert d4 is None and b4 is None and (e4.cpu().numpy() == sc.replay_ref(p, window_bars=W)[0]).all()


def carried(p, s, back, from_t, first=0, bump=0, **kw):
    """Row s alone, from from_t, with the spike of candle from_t - back
    carried in (its open time moved by `bump` ms): kernel and restatement."""
    one = {k: v[s:s + 1] for k, v in p.items()}
    src = from_t - back
    state = (np.ones(1, np.uint8), one["open_time"][:, src] + bump, one["high"][:, src], one["close"][:, src])
    kw = dict(first_t=[first], from_t=[from_t], **kw)
    want = sc.replay_ref(one, state=state, **kw)
    got, st = replay(one, state=state, **kw)
    sc.assert_replay_equal(got, want, f"row {s} back {back}")
    sc.assert_state_equal(st, want[3], f"row {s} back {back}")
    return want, state


def test_carried_in_state(cuda):
    """A spike carried into the launch: found within the window, found
    beyond it, not found, found before first_t, and equal to from_t."""
    T = 200
    p = sc.edge_panel(6, T, seed=11)
    p["source_ok"][:] = False   # only the carried-in spike acts
    quiet = np.maximum(p["open"], p["close"])
    for from_t in (70, 64, 128, 133):
        for s in (3, 4):
            p["high"][s] = quiet[s] * 1.0001   # no extension: the spike waits
            want, state = carried(p, s, 3, from_t)   # within the window
            assert want[0][0, from_t] in (ref.FS_WAITING, ref.FS_CANDIDATE) and want[2][0, from_t] == 3
            p["high"][s, from_t - 2] *= 1.2   # a candle this launch does not replay extends beyond the spike
            want, _ = carried(p, s, 3, from_t)
            assert want[0][0, from_t] == ref.FS_CLEARED and want[1][0, from_t] == ref.D_EXTENSION
            p["high"][s, from_t - 2] = np.nan   # missing: skipped
            want, _ = carried(p, s, 3, from_t)
            assert want[0][0, from_t] != ref.FS_CLEARED
            want, _ = carried(p, s, 8, from_t)
            assert want[2][0, from_t] == 8 and want[0][0, from_t] != ref.FS_CLEARED
            for back in (9, 40, 63, 64):   # beyond the window, up to a whole step back
                want, _ = carried(p, s, back, from_t)
                assert want[0][0, from_t] == ref.FS_CLEARED and want[1][0, from_t] == ref.D_WINDOW_EXPIRED
                assert want[2][0, from_t] == back
            want, _ = carried(p, s, 3, from_t, bump=-1)   # an open time no candle has
            assert want[0][0, from_t] == ref.FS_CLEARED and want[1][0, from_t] == ref.D_CANDLE_EXPIRED
            want, _ = carried(p, s, 3, from_t, first=from_t - 2)   # its candle lies before the frame
            assert want[0][0, from_t] == ref.FS_CLEARED and want[1][0, from_t] == ref.D_CANDLE_EXPIRED
            want, _ = carried(p, s, 3, from_t, first=from_t - 3)   # the frame's first candle
            assert want[1][0, from_t] != ref.D_CANDLE_EXPIRED and want[2][0, from_t] == 3
            want, state = carried(p, s, 0, from_t, lens=[from_t + 1])   # the same candle again: state untouched
            assert want[0][0, from_t] == ref.FS_SAME_CANDLE and want[3][0][0] and want[3][1][0] == state[1][0]
            want, _ = carried(p, s, 0, from_t)   # and the candles after it count from it
            assert want[0][0, from_t] == ref.FS_SAME_CANDLE and want[2][0, from_t + 1] == 1
    want, _ = carried(p, 3, 150, 199)   # a long way back: bars saturates
    assert want[1][0, 199] == ref.D_WINDOW_EXPIRED and want[2][0, 199] == 150
    long = sc.edge_panel(1, 400, seed=12)
    long["source_ok"][:] = False
    want, _ = carried(long, 0, 300, 399)
    assert want[1][0, 399] == ref.D_WINDOW_EXPIRED and want[2][0, 399] == ref.BARS_MAX


@pytest.mark.parametrize("T,k", [(129, 63), (129, 64), (129, 65), (1025, 960), (1025, 1024)])
def test_split_run_equals_whole(cuda, T, k):
    """[0, k) then [k, T) with the carried state, k at and around step edges,
    equals the whole run."""
    S = 6
    p = sc.edge_panel(S, T, seed=1000 + T)
    whole, st_whole = replay(p, state=sc.idle_state(S))
    head, st_head = replay(p, state=sc.idle_state(S), lens=np.full(S, k))
    tail, st_tail = replay(p, state=st_head, from_t=np.full(S, k))
    sc.assert_replay_equal(head, whole, "head", slice(0, k))
    sc.assert_replay_equal(tail, whole, "tail", slice(k, None))
    assert (head[0][:, k:] == ref.FS_NO_FRAME).all() and (tail[0][:, :k] == ref.FS_NO_FRAME).all()
    sc.assert_state_equal(st_tail, st_whole, "carry-out")
    assert st_head[0].any() and (whole[0] == ref.FS_CANDIDATE).sum() >= 5
    sc.assert_replay_equal(whole, sc.replay_ref(p), "whole vs restatement")


def test_shared_and_absent_market_masks(cuda):
    """ld_m == 0: one [T] row shared by all symbols equals the expanded
    [S, T] masks; no masks equal masks of ones."""
    S, T = 9, 200
    p = sc.edge_panel(S, T, seed=21)
    shared = {**p, "src_market": p["src_market"][2], "fail_market": p["fail_market"][2]}
    expanded = {**p, "src_market": np.tile(p["src_market"][2], (S, 1)), "fail_market": np.tile(p["fail_market"][2], (S, 1))}
    from binquant_amd import engine

    cols = [dv(p[k]) for k in sc.COLS + ("open_time", "source_ok")]
    got = host(engine.spike_fade_replay(*cols, dv(shared["src_market"]), dv(shared["fail_market"])))
    want, _ = replay(expanded)
    sc.assert_replay_equal(got, want, "shared row")
    sc.assert_replay_equal(got, sc.replay_ref(shared), "shared row vs restatement")
    one_sided = host(engine.spike_fade_replay(*cols, None, dv(shared["fail_market"])))
    sc.assert_replay_equal(one_sided, sc.replay_ref({**shared, "src_market": None}), "failure gate only")
    none, _ = replay(p, masks=False)
    ones = {**p, "src_market": np.ones((S, T), bool), "fail_market": np.ones((S, T), bool)}
    sc.assert_replay_equal(none, replay(ones)[0], "no masks")
    sc.assert_replay_equal(none, sc.replay_ref({**p, "src_market": None, "fail_market": None}), "no masks vs restatement")


def test_allow_helpers_equal_reference(cuda):
    """signals.spike_source_allows / spike_fade_market_allows against the
    real methods over the fixture's grids and its per-candle recordings: ok
    and reason, exact."""
    from binquant_amd import signals

    fx, p = sc.fixture(), sc.panel()
    g = pg.source_cases()
    n = len(g["label"])
    ok, reason = signals.spike_source_allows(*(dv(g[k]).reshape(1, n) for k in sc.SPIKE_FIELDS))
    assert ok.dtype == torch.bool and reason.dtype == torch.uint8 and tuple(ok.shape) == (1, n)
    assert (reason.cpu().numpy()[0] == fx["grid_spike_reason"]).all() and (ok.cpu().numpy()[0] == fx["grid_spike_ok"]).all()
    ok, reason = signals.spike_source_allows(*(dv(fx[f"spike_{k}"]) for k in sc.SPIKE_FIELDS))
    inside = (np.arange(pg.T) >= p["first_t"][:, None]) & (np.arange(pg.T) < p["lens"][:, None])
    assert (reason.cpu().numpy() == fx["source_reason"])[inside].all()
    assert (ok.cpu().numpy() == fx["source_ok"])[inside].all()
    m = pg.market_cases()
    res = signals.spike_fade_market_allows(*(dv(m[k]) for k in ("stress", "long_score", "short_score", "context_ok",
                                                                "momentum")))
    for x, k in zip(res, ("grid_src_ok", "grid_src_reason", "grid_fail_ok", "grid_fail_reason")):
        assert tuple(x.shape) == (len(m["stress"]),) and (x.cpu().numpy() == fx[k]).all(), k
    assert res[0].dtype == torch.bool and res[1].dtype == torch.uint8
    s = 5   # one row's context, candle by candle
    res = signals.spike_fade_market_allows(*(dv(p[k][s]) for k in ("stress", "long_score", "short_score", "context_ok",
                                                                   "momentum")))
    for x, k in zip(res, ("src_market", "src_market_reason", "fail_market", "fail_market_reason")):
        assert (x.cpu().numpy() == fx[k][s]).all(), k


def test_signals_end_to_end(cuda):
    """signals.failed_spike_fade on the fixture rows, and the cohort's claim:
    the device failed_spike_features (exact=True) of the frame ending at t,
    its newest column fed through spike_source_allows, is the recorded
    source_ok of candle t — on source candles and on others."""
    from binquant_amd import signals, strategies

    fx, p = sc.fixture(), sc.panel()
    inp = sc.fixture_inputs()
    state = signals.SpikeFadeState.idle(pg.S, "cuda")
    res = signals.failed_spike_fade(*(dv(inp[k]) for k in sc.COLS + ("open_time", "source_ok")),
                                    src_market=dv(inp["src_market"]), fail_market=dv(inp["fail_market"]), state=state,
                                    first_t=dv(p["first_t"]), lens=dv(p["lens"]), from_t=dv(p["first_t"]))
    assert list(res) == ["event", "detail", "bars"]
    sc.assert_replay_equal(host(res.values()), (fx["event"], fx["detail"], fx["bars"]), "signals")
    sc.assert_state_equal(host(state.tensors()), sc.recorded_state(p["lens"] - 1), "signals state")
    rows = np.array([0, 4, 7, 10, 13, 16])   # frames from candle 0, full length
    assert (p["first_t"][rows] == 0).all() and (p["lens"][rows] == pg.T).all()
    set_at = np.unique(np.nonzero(fx["source_ok"][rows])[1])
    ends = np.unique(np.r_[set_at[::7], set_at[::7] + 1, 60, 199])
    trues = 0
    for t in ends:
        f = strategies.failed_spike_features(*(dv(p[k][rows, :t + 1]) for k in ("open", "high", "low", "close", "volume",
                                                                                "quote_asset_volume")), exact=True)
        ok, reason = signals.spike_source_allows(*(f[k] for k in sc.SPIKE_FIELDS))
        assert (ok[:, -1].cpu().numpy() == fx["source_ok"][rows, t]).all(), t
        assert (reason[:, -1].cpu().numpy() == fx["source_reason"][rows, t]).all(), t
        trues += int(fx["source_ok"][rows, t].sum())
    assert trues >= 5 and len(ends) <= 16


def cohort_inputs(p, p5, rows, window):
    five = [dv(p5[k]) for k in ("open", "high", "low", "close", "volume")]
    btc = 60000.0 * np.exp(np.cumsum(np.random.default_rng(5).normal(0.0, 0.001, pg.T)))
    return five + [dv(p[k][rows, window]) for k in ("open", "high", "low", "close", "volume", "open_time")] + [
        dv(p["open_time"][0, window]), dv(btc[window])]


def test_cohort_spike_fade_candle_by_candle(cuda):
    """process_cohort(spike_fade=state) fed 30 growing prefixes of 8 fixture
    rows equals the recording, the source gate formed from the cohort's own
    spike.* columns; without a state its outputs are the same dict as before."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.synth import numpy_panel

    fx, p = sc.fixture(), sc.panel()
    rows, t_first, n = np.arange(8), 120, 30
    p5 = numpy_panel(len(rows), 200, seed0=3, edges=True)
    state = signals.SpikeFadeState(*device_state(sc.recorded_state(np.full(len(rows), t_first - 1), rows)))
    ev, dt, br = (np.empty((len(rows), n), np.uint8) for _ in range(3))
    for i in range(n):
        t = t_first + i
        masks = tuple(dv(np.ascontiguousarray(fx[k][rows, :t + 1])) for k in ("src_market", "fail_market"))
        out = process_cohort(*cohort_inputs(p, p5, rows, slice(0, t + 1)), spike_fade=state, spike_fade_market=masks)
        ev[:, i], dt[:, i], br[:, i] = (out[f"spikefade.{k}"].cpu().numpy() for k in ("event", "detail", "bars"))
    cols = slice(t_first, t_first + n)
    sc.assert_replay_equal((ev, dt, br), tuple(fx[k][rows, cols] for k in ("event", "detail", "bars")), "cohort")
    sc.assert_state_equal(host(state.tensors()), sc.recorded_state(np.full(len(rows), t_first + n - 1), rows),
                          "cohort state")
    assert len(np.unique(ev)) >= 5
    plain = process_cohort(*cohort_inputs(p, p5, rows, slice(0, 150)))
    with_state = process_cohort(*cohort_inputs(p, p5, rows, slice(0, 150)),
                                spike_fade=signals.SpikeFadeState.idle(len(rows), "cuda"))
    assert not any(k.startswith("spikefade.") for k in plain)
    assert [k for k in with_state if k not in plain] == ["spikefade.event", "spikefade.detail", "spikefade.bars"]
    for k in plain:
        a, b = plain[k], with_state[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k


def test_cohort_defaults_unchanged(cuda):
    """process_cohort without spike_fade returns the keys it returned before
    (no spikefade.* and, by the other options' defaults, no impulse.* /
    ladder.* / retest.* / topentry.*)."""
    from binquant_amd.cohort import process_cohort
    from binquant_amd.synth import numpy_panel

    p = sc.panel()
    rows = np.arange(4)
    out = process_cohort(*cohort_inputs(p, numpy_panel(len(rows), 200, seed0=3, edges=True), rows, slice(0, 150)))
    stages = {k.split(".")[0] for k in out}
    assert stages == {"e5", "burst", "e15", "h1", "btc", "context", "pump", "spike", "top", "lead"}, stages


def test_cohort_captured_graph_carries_state(cuda):
    """The cohort with pending spikes captured as one graph (the number of
    hardware queues as the machine sets it): the state tensors are updated in
    place by every replay (set after the capture, whose warm-up calls advance
    them). The first message is a fixture prefix frame on which some row sets
    its spike: the replay equals the recording; the same frame replayed again
    gives SAME_CANDLE on that row and leaves the state; two further messages
    equal eager ones — outputs and state."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline
    from binquant_amd.synth import numpy_panel

    fx, p = sc.fixture(), sc.panel()
    rows = np.arange(8)
    set_cols = np.nonzero(fx["event"][rows] == ref.FS_SOURCE_SET)[1]
    t_s = int(set_cols[set_cols >= 100].min())
    T = t_s + 1
    p5 = numpy_panel(len(rows), 200, seed0=3, edges=True)
    inputs = lambda end: cohort_inputs(p, p5, rows, slice(end - T, end))   # noqa: E731
    start = sc.recorded_state(np.full(len(rows), t_s - 1), rows)
    eager_state, graph_state = (signals.SpikeFadeState(*device_state(start)) for _ in range(2))
    masks = tuple(dv(np.ascontiguousarray(fx[k][rows, :T])) for k in ("src_market", "fail_market"))

    def set_masks(end):
        for m, k in zip(masks, ("src_market", "fail_market")):
            m.copy_(dv(np.ascontiguousarray(fx[k][rows, end - T:end])))

    graph = CapturedPipeline(functools.partial(process_cohort, spike_fade=graph_state, spike_fade_market=masks),
                             *inputs(T))
    for dst, src in zip(graph_state.tensors(), device_state(start)):
        dst.copy_(src)
    got = graph(*inputs(T))
    torch.cuda.synchronize()
    first = got["spikefade.event"].cpu().numpy()
    for k in ("event", "detail", "bars"):
        assert (got[f"spikefade.{k}"].cpu().numpy() == fx[k][rows, t_s]).all(), k
    after = sc.recorded_state(np.full(len(rows), t_s), rows)
    sc.assert_state_equal(host(graph_state.tensors()), after, "after the first message")
    pending = after[0].astype(bool)
    assert (first == ref.FS_SOURCE_SET).any()
    got = graph(*inputs(T))   # the same frame again
    torch.cuda.synchronize()
    again = got["spikefade.event"].cpu().numpy()
    assert (again[first == ref.FS_SOURCE_SET] == ref.FS_SAME_CANDLE).all()
    assert (again[pending & (first != ref.FS_SOURCE_SET)] == first[pending & (first != ref.FS_SOURCE_SET)]).all()
    sc.assert_state_equal(host(graph_state.tensors()), after, "after the repeat")
    for dst, src in zip(eager_state.tensors(), device_state(after)):
        dst.copy_(src)
    for end in (T + 1, T + 2):
        set_masks(end)
        want = process_cohort(*inputs(end), spike_fade=eager_state, spike_fade_market=masks)
        want = {k: want[f"spikefade.{k}"].clone() for k in ("event", "detail", "bars")}
        got = graph(*inputs(end))
        torch.cuda.synchronize()
        for k in ("event", "detail", "bars"):
            assert torch.equal(got[f"spikefade.{k}"], want[k]), (end, k)
        sc.assert_state_equal(host(graph_state.tensors()), host(eager_state.tensors()), f"message {end}")


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    p = sc.edge_panel(6, 130, seed=1)
    good = [dv(p[k]) for k in sc.COLS + ("open_time", "source_ok")]
    for kw in (dict(window_bars=0), dict(window_bars=33)):
        with pytest.raises(ValueError, match="window_bars"):
            engine.spike_fade_replay(*good, **kw)
    with pytest.raises(ValueError, match="ext_factor"):
        engine.spike_fade_replay(*good, ext_factor=float("inf"))
    for i, bad in ((1, good[1].float()), (2, good[2][:, :-1]), (3, good[3].int()), (4, good[4].to(torch.uint8)),
                   (0, good[0].cpu())):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            engine.spike_fade_replay(*args)
    with pytest.raises(ValueError):
        engine.spike_fade_replay(*good, dv(p["src_market"]).cpu())
    with pytest.raises(ValueError):
        engine.spike_fade_replay(*good, state=(dv(np.zeros(6, np.uint8)), dv(np.zeros(6, np.int32)), dv(np.zeros(6)),
                                               dv(np.zeros(6))))
