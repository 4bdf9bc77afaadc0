"""FailedSpikeFade.latest_signal() at every candle on the device
(strategies.failed_spike_frames / engine.spike_frames, bq_spikeframes.hip):
against what a fresh instance of the REAL class returned on every frame
(tests/golden/spikeframes.npz), against the last_spike fields of the
pending-spike fixture (spikefade_gates.npz), against the library's own exact
route (one failed_spike_features call per frame) and, at the kernel's edges,
against the numpy restatement those fixtures pin (tests/spikeframes_ref.py).

Booleans are exact everywhere. The two thresholds: within 1e-9 relative of
the fixture and the restatement (SURVEY §8c's bar: they are lerps of the
device-formed volume_ratio), bit-equal to failed_spike_features(exact=True)
of the same frame (same keys, same shared lerp helper)."""

import functools

import numpy as np
import pytest
import torch

from tests import spikeframes_cases as sc
from tests.spikeframes_cases import pg, ref

pytestmark = pytest.mark.gpu

THRESHOLDS = ("volume_cluster_min_ratio", "price_break_base_threshold")
RTOL = 1e-9


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


def assert_thresholds_close(got, want, mask, what):
    for k in THRESHOLDS:
        g, w = got[k][mask], want[k][mask]
        err = np.abs(g - w) / np.abs(w)
        assert np.isfinite(g).all() and (err <= RTOL).all(), f"{what}: {k} off by {np.nanmax(err):.3g} relative"


def assert_matches_ref(got, want, mask, what):
    sc.assert_bools_equal(got, want, mask, what)
    assert_thresholds_close(got, want, mask, what)
    assert sc.same_bits(got["close_open_ratio"][mask], want["close_open_ratio"][mask]).all(), what
    sc.assert_fill(got, mask, what)


@functools.lru_cache(maxsize=1)
def device_fixture():
    p = sc.panel()
    return frames(p, first_t=p["first_t"], lens=p["lens"])


def test_fixture_parity(cuda):
    """Every flag of every in-frame cell equals the fresh instance's; the
    thresholds within 1e-9 relative; the fill outside."""
    fx, p = sc.fixture(), sc.panel()
    mask = sc.in_frame(p)
    got = device_fixture()
    assert list(got) == list(ref.BOOL_KEYS[:12]) + list(THRESHOLDS) + ["close_open_ratio"]
    assert_matches_ref(got, fx, mask, "fixture")
    # what the fixture is for, counted on the device's own output
    assert (got["label_pre"] & ~got["label"]).sum() >= 50 and (fx["walk"][got["label_pre"]] > 128).sum() >= 3
    assert (got["price_break_base_threshold"][mask] > 0.03).sum() >= 100
    assert (got["volume_cluster_min_ratio"][mask] == 1.15).sum() >= 5
    assert ((got["volume_cluster_min_ratio"] == 1.6) & mask).sum() >= 10


def test_second_fixture_and_source_gate(cuda):
    """spikefade_gates.npz's recorded last_spike fields, source_ok and
    source_reason: all 4569 cells, through signals.spike_source_frames."""
    from binquant_amd import signals

    fx, p = sc.fade_fixture(), sc.fade_panel()
    mask = sc.in_frame(p)
    got = frames(p, first_t=p["first_t"], lens=p["lens"])
    for k in sc.FADE_FIELDS:
        assert (got[k][mask] == fx[f"spike_{k}"][mask].astype(bool)).all(), k
    assert sc.same_bits(got["close_open_ratio"][mask], fx["spike_close_open_ratio"][mask]).all()
    ok, reason = signals.spike_source_frames(*(dv(p[k]) for k in sc.OHLCV), first_t=dv(p["first_t"]),
                                             lens=dv(p["lens"]))
    ok, reason = ok.cpu().numpy(), reason.cpu().numpy()
    assert mask.sum() == 4569
    assert (ok[mask] == fx["source_ok"][mask]).all() and (reason[mask] == fx["source_reason"][mask]).all()
    assert not ok[~mask].any()


ROWS_A = (0, 1, 3, 8, 9)   # frames from candle 0, full length
ENDS = ([(ROWS_A, 0, t) for t in (0, 10, 11, 12, 19, 20, 59, 60, 159, 160, 173, 287)]
        + [((5,), 37, 37 + d) for d in (0, 11, 12, 60, 159, 250)] + [((6,), 0, 200), ((7,), 100, 108)])


def test_kernel_equals_per_frame_exact_route(cuda):
    """Column t against failed_spike_features(frame ending at t, exact=True)'s
    newest column: the flags equal, the two thresholds BIT-equal."""
    from binquant_amd import strategies

    p = sc.panel()
    got = device_fixture()
    assert len(ENDS) <= 24 and len({s for rows, _, _ in ENDS for s in rows}) <= 8
    labels = 0
    for rows, first, t in ENDS:
        rows = np.array(rows)
        assert (p["first_t"][rows] == first).all() and (t < p["lens"][rows]).all()
        f = strategies.failed_spike_features(*(dv(p[k][rows, first:t + 1]) for k in sc.OHLCV), exact=True)
        for k in ref.BOOL_KEYS:
            assert (f[k][:, -1].cpu().numpy() == got[k][rows, t]).all(), (k, rows, t)
        for k in THRESHOLDS:   # per row there: the frame's calibrated values
            assert sc.same_bits(f[k].cpu().numpy(), got[k][rows, t]).all(), (k, rows, t)
        assert sc.same_bits(f["close_open_ratio"][:, -1].cpu().numpy(), got["close_open_ratio"][rows, t]).all()
        labels += int(got["label_pre"][rows, t].sum())
    assert labels >= 3


EDGE_T = (1, 11, 12, 63, 64, 65, 129)
EDGE_S = (1, 5, 65)


@pytest.mark.parametrize("T", EDGE_T)
def test_shapes_vs_restatement(cuda, T):
    """Rows per workgroup not filled, more than one workgroup, frames that end
    inside, at and just past a 64-candle step, frames shorter than the
    calibration's warm-up."""
    for S in EDGE_S:
        p = sc.synth_panel(S, T, seed=7000 + 10 * T + S)
        want = ref.frames(p["open"], p["close"], p["volume"], back_walk=True)
        assert_matches_ref(frames(p), want, np.ones((S, T), bool), f"S={S} T={T}")


@pytest.mark.parametrize("kind", ["nan", "equal", "dense5", "ragged"])
def test_special_rows_vs_restatement(cuda, kind):
    """An all-NaN panel (no observation: the defaults everywhere), equal
    candles (ties in the ranking), a label every 5 bars for 200 bars (the
    back-walk crosses three 64-candle blocks to the frame's first row), and
    ragged rows: first_t no multiple of 64, lens < T, fewer candles than
    base_window."""
    S, T = 5, 230
    p = sc.synth_panel(S, T, seed=91, kind="mixed" if kind == "ragged" else kind)
    first = np.array([0, 37, 70, 129, 215]) if kind == "ragged" else None
    lens = np.array([230, 201, 230, 190, 224]) if kind == "ragged" else None
    walks = []
    want = ref.frames(p["open"], p["close"], p["volume"], first_t=first, lens=lens, back_walk=True, walks=walks)
    got = frames(p, first_t=first, lens=lens)
    mask = np.ones((S, T), bool) if first is None else (np.arange(T) >= first[:, None]) & (np.arange(T) < lens[:, None])
    assert_matches_ref(got, want, mask, kind)
    if kind == "nan":
        assert (got["volume_cluster_min_ratio"] == 1.6).all() and (got["price_break_base_threshold"] == 0.03).all()
        assert not got["label_pre"].any()
    if kind == "dense5":
        assert max(walks) > 192 and (got["label_pre"] & ~got["label"]).sum() >= 20 and got["label"].sum() >= 20


@pytest.mark.parametrize("mode,bars,both", [("first", 8, False), ("all", 3, False), ("last", 0, True),
                                            ("last", 63, False)])
def test_label_modes_and_cooldowns(cuda, mode, bars, both):
    """The other cluster label modes, require_both_patterns, no cooldown and
    the longest one, with a lower volume quantile so that clusters are common."""
    from binquant_amd import strategies

    p = sc.synth_panel(4, 150, seed=17)
    kw = dict(volume_cluster_label_mode=mode, post_spike_cooldown_bars=bars, require_both_patterns=both,
              volume_quantile=0.8)
    want = ref.frames(p["open"], p["close"], p["volume"], ref.Params(**kw), back_walk=True)
    got = frames(p, strategies.SpikeParams(**kw))
    assert_matches_ref(got, want, np.ones((4, 150), bool), f"{mode} {bars}")
    assert got["volume_cluster_flag"].sum() >= 10
    if bars == 0:
        assert (got["label"] == got["label_pre"]).all() and got["label"].any()


def test_from_t(cuda):
    """from_t = lens - 1 (the live call) equals the full run's newest column;
    a run split at an arbitrary from_t equals the whole run; untouched cells
    keep the fill."""
    p = sc.panel()
    full = device_fixture()
    rows = np.arange(pg.S)
    live = frames(p, first_t=p["first_t"], lens=p["lens"], from_t=p["lens"] - 1)
    newest = np.zeros((pg.S, pg.T), bool)
    newest[rows, p["lens"] - 1] = True
    split_at = np.array([100, 64, 1, 257, 130, 20, 200, 104, 63, 0])
    tail = frames(p, first_t=p["first_t"], lens=p["lens"], from_t=split_at)
    tail_mask = sc.in_frame(p) & (np.arange(pg.T) >= split_at[:, None])
    assert tail_mask.sum() > 1000 and (~tail_mask & sc.in_frame(p)).sum() > 500
    for got, mask, what in ((live, newest, "live"), (tail, tail_mask, "split")):
        for k in ref.BOOL_KEYS:
            assert (got[k][mask] == full[k][mask]).all(), (what, k)
        for k in THRESHOLDS:
            assert sc.same_bits(got[k][mask], full[k][mask]).all(), (what, k)
        sc.assert_fill(got, mask, what)


def test_column_subsets_write_the_same_bits(cuda):
    p = sc.panel()
    full = device_fixture()
    for columns in (("label",), ("price_break_base_threshold", "label_short", "close_open_ratio"),
                    ("volume_cluster_min_ratio",), ("upward", "label_pre", "cumulative_price_break_short_flag")):
        got = frames(p, first_t=p["first_t"], lens=p["lens"], columns=columns)
        assert set(got) == set(columns)
        for k in columns:
            assert sc.same_bits(got[k], full[k]).all() if got[k].dtype == np.float64 else (got[k] == full[k]).all(), k


def test_padded_row_pitch(cuda):
    """engine.spike_frames on columns that are views into wider buffers."""
    from binquant_amd import engine, strategies

    p = sc.synth_panel(5, 100, seed=3)
    o, c, v = (dv(p[k]) for k in ("open", "close", "volume"))
    cols = strategies.spike_frame_columns(o, c, v)
    plain = host(engine.spike_frames(cols, strategies.SpikeParams()))

    def padded(x, pad):
        buf = torch.full((x.shape[0], x.shape[1] + pad), 7, dtype=x.dtype, device=x.device)
        buf[:, :x.shape[1]] = x
        return buf[:, :x.shape[1]]

    wide = {k: padded(x, 24 if x.dtype == torch.bool else 9) for k, x in cols.items()}
    assert wide["close"].stride(0) == 109 and wide["upward"].stride(0) == 124
    got = host(engine.spike_frames(wide, strategies.SpikeParams()))
    for k in plain:
        assert sc.same_bits(got[k], plain[k]).all() if got[k].dtype == np.float64 else (got[k] == plain[k]).all(), k
    assert plain["label_pre"].any()


def test_end_to_end_source_gate_into_the_replay(cuda):
    """signals.spike_source_frames -> signals.failed_spike_fade on the new
    fixture equals the pending-spike restatement fed the source gate the real
    class recorded on every frame."""
    import spikefade_ref
    from binquant_amd import signals

    fx, p = sc.fixture(), sc.panel()
    ok, _ = signals.spike_source_frames(*(dv(p[k]) for k in sc.OHLCV), first_t=dv(p["first_t"]), lens=dv(p["lens"]))
    res = signals.failed_spike_fade(dv(p["open"]), dv(p["high"]), dv(p["close"]), dv(p["open_time"]), ok,
                                    first_t=dv(p["first_t"]), lens=dv(p["lens"]))
    recorded_ok, _ = ref.source_allows(fx, float(fx["max_candle_return"]))
    want = spikefade_ref.spike_fade_replay(p["open"], p["high"], p["close"], p["open_time"], recorded_ok,
                                           first_t=p["first_t"], lens=p["lens"])
    for name, w in zip(("event", "detail", "bars"), want[:3]):
        assert (res[name].cpu().numpy() == w).all(), name
    assert recorded_ok.sum() >= 5 and (want[0] == spikefade_ref.FS_SOURCE_SET).sum() >= 5


def test_capture_replays_bit_equal(cuda):
    """One capture of the whole pass (no device read-back, shape-only
    allocations); a replay on other inputs equals the eager call."""
    from binquant_amd import strategies
    from binquant_amd.graphs import CapturedPipeline

    a, b = sc.synth_panel(6, 150, seed=5), sc.synth_panel(6, 150, seed=6)
    first = dv(np.array([0, 5, 64, 70, 0, 130], np.int64))

    def fn(o, h, l, c, v, qv):
        return strategies.failed_spike_frames(o, h, l, c, v, qv, first_t=first)

    pipe = CapturedPipeline(fn, *(dv(a[k]) for k in sc.OHLCV))
    got = {k: x.clone() for k, x in pipe(*(dv(b[k]) for k in sc.OHLCV)).items()}
    torch.cuda.synchronize()
    eager = fn(*(dv(b[k]) for k in sc.OHLCV))
    for k in eager:
        g, w = got[k].cpu().numpy(), eager[k].cpu().numpy()
        assert sc.same_bits(g, w).all() if g.dtype == np.float64 else (g == w).all(), k
    assert eager["label_pre"].any()
