"""FailedSpikeFade.latest_signal() under a sliding frame cap on the device
(strategies.failed_spike_frames(frame_cap=M) / engine.spike_frames,
bq_spike_frames_capped): against what a fresh instance of the REAL class
returned on every capped frame (tests/golden/spikecap.npz, M = 64, 96, 301)
and, at the kernels' edges, against the slow restatement that fixture pins
(tests/spikecap_ref.py: one cut-out frame per cell).

Booleans are exact everywhere; every random case first asserts that its
oracle sees no comparison within 1e-9 relative of a tie. The two thresholds:
within 1e-9 relative (SURVEY §8c's bar for fp64 against pandas; observed
~1e-15): pandas sums a capped frame's rolling mean from the frame's first
row, the column stage from the row's, so bit-equality cannot hold."""

import functools

import numpy as np
import pytest
import torch

from tests import spikecap_cases as sc
from tests.spikecap_cases import pg, ref

pytestmark = pytest.mark.gpu


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(d):
    return {k: x.cpu().numpy() for k, x in d.items()}


def frames(p, params=None, **kw):
    """strategies.failed_spike_frames on a numpy panel -> numpy dict."""
    from binquant_amd import strategies

    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    return host(strategies.failed_spike_frames(*(dv(p[k]) for k in sc.OHLCV), params, **kw))


def same(got, want, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        assert sc.same_bits(g, w).all() if g.dtype == np.float64 else (g == w).all(), k


@functools.lru_cache(maxsize=4)
def device_fixture(cap):
    p = sc.panel()
    return frames(p, first_t=p["first_t"], lens=p["lens"], frame_cap=cap)


@pytest.mark.parametrize("cap", pg.CAPS)
def test_fixture_parity(cuda, cap):
    """Every flag of every in-frame cell equals the fresh instance's on the
    capped frame; the thresholds within 1e-9 relative; the fill outside."""
    fx, mask = sc.recorded(cap), sc.in_frame(sc.panel())
    got = device_fixture(cap)
    assert list(got) == list(ref.BOOL_KEYS[:12]) + list(sc.THRESHOLDS) + ["close_open_ratio"]
    sc.assert_matches(got, fx, mask, f"fixture, cap {cap}")
    # what the fixture is for, counted on the device's own output
    expanding = frames(sc.panel(), first_t=sc.panel()["first_t"], lens=sc.panel()["lens"])
    differs = np.zeros_like(mask)
    for k in ("label", "price_break_flag", "cumulative_price_break_flag"):
        differs |= (got[k] != expanding[k]) & mask
    assert differs.sum() >= (20 if cap == 64 else 1)
    slid = mask & (np.arange(pg.T) >= (sc.panel()["first_t"] + cap)[:, None])
    walk_start = np.arange(pg.T) - fx["walk"]
    in_zone = slid & got["label_pre"] & (walk_start < (np.arange(pg.T) + 1 - cap) + 60)
    assert in_zone.sum() >= (20 if cap == 64 else 0)


EDGE_CAPS = (64, 65, 127, 128, 129)
EDGE_S = (1, 5, 65)


def edge_T(cap):
    return (cap - 1, cap, cap + 1, cap + 64, 2 * cap + 3)


@pytest.mark.parametrize("cap", EDGE_CAPS)
def test_shapes_vs_restatement(cuda, cap):
    """Caps at, just past and just below a multiple of the 64-key chunk;
    frames that never slide, slide once, by a whole step and past two caps;
    rows per workgroup not filled and more than one workgroup (row s of the
    wide panels is row s % 5 of the five-row one: one oracle per shape)."""
    for T in edge_T(cap):
        p = sc.synth_panel(5, T, seed=9000 + 10 * T + cap)
        want = sc.oracle(p, cap)
        for S in EDGE_S:
            q = sc.tiled(p, S)
            w = sc.tiled(want, S)
            sc.assert_matches(frames(q, frame_cap=cap), w, np.ones((S, T), bool), f"cap={cap} S={S} T={T}")


def test_long_row_past_the_uncapped_limit(cuda):
    """T = 2113 > engine.SPIKE_FRAMES_MAX_T: impossible without a cap. About 60
    sampled ends and the last 70 against the oracle."""
    from binquant_amd import engine

    S, T, cap = 2, 2113, 64
    assert T > engine.SPIKE_FRAMES_MAX_T
    p = sc.synth_panel(S, T, seed=2113)
    ends = sorted(set(np.random.default_rng(1).integers(0, T - 70, 60).tolist()) | set(range(T - 70, T)))
    assert sc.ties(p, cap) == 0
    want = sc.cref.frames(p["open"], p["close"], p["volume"], cap, ends=ends)
    got = frames(p, frame_cap=cap)
    mask = np.zeros((S, T), bool)
    mask[:, ends] = True
    sc.assert_bools_equal(got, want, mask, "T=2113")
    sc.assert_thresholds_close(got, want, mask, "T=2113")
    assert got["label_pre"][mask].sum() >= 5 and np.isfinite(got["volume_cluster_min_ratio"]).all()


SPECIAL_S, SPECIAL_T, SPECIAL_CAP = 5, 230, 64
RAGGED_FIRST, RAGGED_LENS = np.array([0, 37, 70, 129, 215]), np.array([230, 201, 230, 190, 224])


@pytest.mark.parametrize("kind", ["nan", "equal", "ragged"])
def test_special_rows_vs_restatement(cuda, kind):
    """An all-NaN panel (no observation in any frame: the defaults
    everywhere), equal candles (ties in the ranking, equal keys erased), and
    ragged rows: first_t no multiple of 64, lens < T, rows shorter than the
    cap and shorter than base_window."""
    S, T, cap = SPECIAL_S, SPECIAL_T, SPECIAL_CAP
    p = sc.synth_panel(S, T, seed=91, kind="mixed" if kind == "ragged" else kind)
    first = RAGGED_FIRST if kind == "ragged" else None
    lens = RAGGED_LENS if kind == "ragged" else None
    want = sc.oracle(p, cap, first_t=first, lens=lens)
    got = frames(p, first_t=first, lens=lens, frame_cap=cap)
    mask = np.ones((S, T), bool) if first is None else (np.arange(T) >= first[:, None]) & (np.arange(T) < lens[:, None])
    sc.assert_matches(got, want, mask, kind)
    if kind == "nan":
        assert (got["volume_cluster_min_ratio"] == 1.6).all() and (got["price_break_base_threshold"] == 0.03).all()
        assert not got["label_pre"].any()
    if kind == "ragged":
        assert got["label_pre"][mask].sum() >= 10


def test_from_t(cuda):
    """from_t = lens - 1 (the live call: the window is rebuilt by cap - 1
    inserts) equals the full run's newest column bit for bit; so does a run
    split at an arbitrary from_t; untouched cells keep the fill."""
    p, cap = sc.panel(), 96
    full = device_fixture(cap)
    rows = np.arange(pg.S)
    live = frames(p, first_t=p["first_t"], lens=p["lens"], from_t=p["lens"] - 1, frame_cap=cap)
    newest = np.zeros((pg.S, pg.T), bool)
    newest[rows, p["lens"] - 1] = True
    split_at = np.array([100, 64, 1, 257, 130, 20, 419, 104])
    tail = frames(p, first_t=p["first_t"], lens=p["lens"], from_t=split_at, frame_cap=cap)
    tail_mask = sc.in_frame(p) & (np.arange(pg.T) >= split_at[:, None])
    assert tail_mask.sum() > 1000 and (~tail_mask & sc.in_frame(p)).sum() > 500
    for got, mask, what in ((live, newest, "live"), (tail, tail_mask, "split")):
        for k in ref.BOOL_KEYS:
            assert (got[k][mask] == full[k][mask]).all(), (what, k)
        for k in sc.THRESHOLDS:
            assert sc.same_bits(got[k][mask], full[k][mask]).all(), (what, k)
        sc.assert_fill(got, mask, what)


def test_missing_close_at_a_frames_first_row(cuda):
    """The close missing exactly on a capped frame's first row with a valid
    close just before it: alone, in a pair and in a run of six, after which
    the frame's newest row has its rolling quantile cut (g > f + 3)."""
    p, cap = sc.gap_at_frame_start(), 64
    assert np.isnan(p["close"][:, [30, 60, 65, 100, 101]]).all() and np.isfinite(p["close"][:, [29, 59, 99]]).all()
    want = sc.oracle(p, cap)
    got = frames(p, frame_cap=cap)
    sc.assert_matches(got, want, np.ones(p["close"].shape, bool), "gap at the frame's first row")
    # those frames' price floor is not the quantile of the row's own finite changes inside them
    starts_missing = [t for t in range(cap, 200) if np.isnan(p["close"][0, t + 1 - cap])]
    assert len(starts_missing) == 9
    pca = ref.frame_columns(p["open"][2], p["close"][2], p["volume"][2], ref.Params())["price_change_abs"]
    naive = np.array([max(0.03, float(np.nanquantile(pca[t + 2 - cap:t + 1], 0.75))) for t in starts_missing])
    assert (naive != got["price_break_base_threshold"][2, starts_missing]).any()


@pytest.mark.parametrize("bars", [0, 3, 8, 63])
def test_dense_labels_and_cooldowns(cuda, bars):
    """A label every 5 bars for 210 bars: with post_spike_cooldown_bars = 63
    no run of clear rows exists and the walk reaches the capped frame's first
    row; 0 is no cooldown."""
    from binquant_amd import strategies

    S, T, cap = 3, 230, 64
    p = sc.synth_panel(S, T, seed=91, kind="dense5")
    want = sc.oracle(p, cap, ref.Params(post_spike_cooldown_bars=bars))
    got = frames(p, strategies.SpikeParams(post_spike_cooldown_bars=bars), frame_cap=cap)
    sc.assert_matches(got, want, np.ones((S, T), bool), f"dense5 bars={bars}")
    assert got["label_pre"].sum() >= 60
    if bars == 0:
        assert (got["label"] == got["label_pre"]).all()
    elif bars == 3:   # shorter than the spacing: nothing between two spikes is suppressed by the one before
        assert got["label"].sum() >= 60
    else:
        assert (got["label_pre"] & ~got["label"]).sum() >= 20 and got["label"].sum() >= (3 if bars == 63 else 20)
    if bars == 63:   # the restatement's walk from each labelled cell ends on the frame's first row
        c = sc.cref.row_columns(p["open"][0], p["close"][0], p["volume"][0], ref.Params())
        t = 200
        vc, pb = sc.cref._thresholds(c, t + 1 - cap, t, ref.Params())
        pre = sc.cref.local_flags(c, t + 1 - cap, t, vc, pb, ref.Params())[0]["label_pre"]
        assert ref.walk_start(pre[:int(np.nonzero(pre)[0][-1]) + 1], bars) == 0


@pytest.mark.parametrize("mode,both", [("first", False), ("all", False), ("last", True)])
def test_label_modes(cuda, mode, both):
    """The three cluster label modes and require_both_patterns, with a lower
    volume quantile so that clusters are common."""
    from binquant_amd import strategies

    kw = dict(volume_cluster_label_mode=mode, require_both_patterns=both, volume_quantile=0.8)
    p = sc.synth_panel(4, 150, seed=17)
    want = sc.oracle(p, 64, ref.Params(**kw))
    got = frames(p, strategies.SpikeParams(**kw), frame_cap=64)
    sc.assert_matches(got, want, np.ones((4, 150), bool), f"{mode} {both}")
    assert got["volume_cluster_flag"].sum() >= 10


def test_column_subsets_write_the_same_bits(cuda):
    p, cap = sc.panel(), 64
    full = device_fixture(cap)
    for columns in (("label",), ("price_break_base_threshold", "label_short", "close_open_ratio"),
                    ("volume_cluster_min_ratio",), ("upward", "label_pre", "accel_spike_flag")):
        got = frames(p, first_t=p["first_t"], lens=p["lens"], columns=columns, frame_cap=cap)
        assert set(got) == set(columns)
        same(got, full, columns)


def test_padded_row_pitch(cuda):
    """engine.spike_frames(frame_cap=) on columns that are views into wider buffers."""
    from binquant_amd import engine, strategies

    p = sc.synth_panel(5, 150, seed=3)
    o, c, v = (dv(p[k]) for k in ("open", "close", "volume"))
    cols = strategies.spike_frame_columns(o, c, v, cap=True)
    assert cols["dyn_src"].dtype == cols["close_next"].dtype == torch.int32
    plain = host(engine.spike_frames(cols, strategies.SpikeParams(), frame_cap=64))

    def padded(x, pad):
        buf = torch.full((x.shape[0], x.shape[1] + pad), 7, dtype=x.dtype, device=x.device)
        buf[:, :x.shape[1]] = x
        return buf[:, :x.shape[1]]

    wide = {k: padded(x, 24 if x.dtype == torch.bool else 9) for k, x in cols.items()}
    assert wide["close"].stride(0) == 159 and wide["upward"].stride(0) == 174
    same(host(engine.spike_frames(wide, strategies.SpikeParams(), frame_cap=64)), plain)
    assert plain["label_pre"].any()


def test_cap_at_least_T_is_the_uncapped_call(cuda):
    """No frame slides: the uncapped kernels run; flags equal, thresholds bit-equal."""
    p = sc.panel()
    rows = dict(first_t=p["first_t"], lens=p["lens"])
    plain = frames(p, **rows)
    for cap in (pg.T, pg.T + 1, 2048):
        same(frames(p, frame_cap=cap, **rows), plain)
    # and a cap that only just bites differs from it somewhere
    assert not sc.same_bits(device_fixture(301)["volume_cluster_min_ratio"], plain["volume_cluster_min_ratio"]).all()


def test_end_to_end_source_gate_into_the_replay(cuda):
    """signals.spike_source_frames(frame_cap=) -> signals.failed_spike_fade
    equals the pending-spike restatement fed the source gate the real class
    recorded on every capped frame."""
    import spikefade_ref
    from binquant_amd import signals

    p, cap = sc.panel(), 64
    fx = dict(sc.recorded(cap))
    o, c = p["open"], p["close"]
    fx["close_open_ratio"] = (c - o) / (o + 1e-6)
    ok, reason = signals.spike_source_frames(*(dv(p[k]) for k in sc.OHLCV), first_t=dv(p["first_t"]),
                                             lens=dv(p["lens"]), frame_cap=cap)
    recorded_ok, recorded_reason = ref.source_allows(fx)
    mask = sc.in_frame(p)
    assert (ok.cpu().numpy()[mask] == recorded_ok[mask]).all()
    assert (reason.cpu().numpy()[mask] == recorded_reason[mask]).all() and not ok.cpu().numpy()[~mask].any()
    res = signals.failed_spike_fade(dv(p["open"]), dv(p["high"]), dv(p["close"]), dv(p["open_time"]), ok,
                                    first_t=dv(p["first_t"]), lens=dv(p["lens"]))
    want = spikefade_ref.spike_fade_replay(p["open"], p["high"], p["close"], p["open_time"], recorded_ok & mask,
                                           first_t=p["first_t"], lens=p["lens"])
    for name, w in zip(("event", "detail", "bars"), want[:3]):
        assert (res[name].cpu().numpy() == w).all(), name
    assert (recorded_ok & mask).sum() >= 5 and (want[0] == spikefade_ref.FS_SOURCE_SET).sum() >= 5


def test_capture_replays_bit_equal(cuda):
    """One capture of the whole capped pass (no device read-back, shape-only
    allocations); a replay on other inputs equals the eager call."""
    from binquant_amd import strategies
    from binquant_amd.graphs import CapturedPipeline

    a, b = sc.synth_panel(6, 150, seed=5), sc.synth_panel(6, 150, seed=6)
    first = dv(np.array([0, 5, 64, 70, 0, 130], np.int64))

    def fn(o, h, l, c, v, qv):
        return strategies.failed_spike_frames(o, h, l, c, v, qv, first_t=first, frame_cap=64)

    pipe = CapturedPipeline(fn, *(dv(a[k]) for k in sc.OHLCV))
    got = {k: x.clone() for k, x in pipe(*(dv(b[k]) for k in sc.OHLCV)).items()}
    torch.cuda.synchronize()
    same(host(got), host(fn(*(dv(b[k]) for k in sc.OHLCV))))
    assert got["label_pre"].any()
