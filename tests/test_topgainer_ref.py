"""CPU checks of the top-gainer entry gate: the numpy / pandas restatement
(tests/topgainer_ref.py) equals what the REAL reference methods returned
(tests/golden/topgainer_gates.npz, tests/golden/make_golden_topgainer.py) —
status and entry exact, point-wise values bit for bit, ema20 / ema50 / the two
volume ratios / score within tests/util's 1e-9 —, the fixture holds every
code, no decision of the fixture or of the GPU test's seeded panels rests on
a near-tie, and the C ABI and the wrappers reject bad arguments before a
device is touched."""

import numpy as np
import pytest
import torch

from tests import topgainer_cases as tc
from tests.topgainer_cases import pg, ref

SHAPES_S = (1, 3, 70)
SHAPES_T = (1, 57, 58, 59, 1023, 1024, 1025, 1026, 1024 + 96, 2 * 1024 + 5)


def sampled(res, pos, keys):
    take = lambda a: np.take_along_axis(a, pos, axis=1)   # noqa: E731
    return {"status": take(res["status"]), "entry": take(res["entry"]), "score": take(res["score"]),
            "stop_loss_pct": take(res["stop_loss_pct"]), "values": {k: take(res["values"][k]) for k in keys}}


def recorded(fx, name):
    _, keys = tc.RUNS[name]
    return {"status": fx[f"{name}_status"], "entry": fx[f"{name}_entry"], "score": fx[f"{name}_score"],
            "stop_loss_pct": fx[f"{name}_stop"],
            "values": {k: fx[f"{name}_values"][:, :, i] for i, k in enumerate(keys)}}


@pytest.mark.parametrize("name", sorted(tc.RUNS))
def test_restatement_equals_reference_on_panel(name):
    fx, p = tc.fixture(), tc.panel()
    args, kw = tc.run_args(p, name)
    res = ref.top_gainer_entry(*args, **kw)
    tc.assert_entry_equal(sampled(res, fx["positions"], tc.RUNS[name][1]), recorded(fx, name), name)
    ready = res["entry"] == 0
    ready |= (res["entry"] >= 4) & (res["entry"] <= 14)
    for k, v in res["values"].items():   # every candle, not only the sampled ones
        assert (np.isnan(v) == ~ready).all(), k
    cand = (res["status"] == 0) | (res["status"] == ref.RISK_REJECTED)
    assert (np.isnan(res["score"]) == ~cand).all()
    # stop_loss_pct is NaN off the candidates and where Python's min / max keep a NaN ATR
    assert np.isnan(res["stop_loss_pct"][~cand]).all()
    nan_stop = cand & np.isnan(res["stop_loss_pct"])
    assert (np.isnan(p["atr"][nan_stop])).all() and (name == "plain") <= (not nan_stop.any())


def test_fixture_holds_every_code():
    fx = tc.fixture()
    entry = np.bincount(np.r_[fx["qa_entry"].ravel(), fx["plain_entry"].ravel()], minlength=18)
    status = np.bincount(np.r_[fx["qa_status"].ravel(), fx["plain_status"].ravel()], minlength=18)
    assert (entry[:15] >= 10).all() and entry[15:].sum() == 0, entry
    assert (status[:18] >= 10).all() and status[18:].sum() == 0, status
    assert [float(x) for x in fx["defaults"]] == [float(ref.DEFAULTS[k]) for k in fx["default_names"]]
    assert list(fx["default_names"]) == list(ref.DEFAULTS)
    assert (fx["positions"][:, -3:] == pg.T - 1 - np.array([2, 1, 0])).all()   # the last rows are always sampled
    # the clamps of _stop_loss_pct and a NaN / zero ATR all occur among the confirmations
    stop = fx["qa_stop"][fx["qa_status"] == 0]
    assert (stop == 1.5).any() and (stop == 2.0).any() and ((stop > 1.5) & (stop < 2.0)).any() and np.isnan(stop).any()
    assert set(np.unique(fx["plain_stop"][fx["plain_status"] == 0])) == {1.5}   # no ATR column (:420)


def test_no_decision_rests_on_a_near_tie():
    """On the fixture's recorded candles, and on every candle of the seeded
    edge panels of tests/test_topgainer_gpu.py (which may therefore demand
    exact codes of a kernel whose ema / volume-ratio columns agree to 1e-9)."""
    fx, p = tc.fixture(), tc.panel()
    at = np.zeros((pg.S, pg.T), bool)
    np.put_along_axis(at, fx["positions"], True, axis=1)
    for name in tc.RUNS:
        args, kw = tc.run_args(p, name)
        assert tc.near_ties(*args, first_t=kw["first_t"], at=at) == 0, name
    for S in SHAPES_S:
        for T in SHAPES_T:
            q = tc.injected_panel(S, T, seed=1000 * S + T)
            for qa in (True, False):
                extra = (q["quote_volume"], q["atr"]) if qa else (None, None)
                assert tc.near_ties(*(q[k] for k in tc.INPUTS), *extra) == 0, (S, T, qa)


def test_restatement_equals_reference_on_frames():
    """The reference test's breakout frame confirms; its short-history frame
    confirms on a 61-bar extension window; each mutation gives its reason."""
    fx = tc.fixture()
    names = [str(n) for n in fx["frame_names"]]
    got = {}
    for i, name in enumerate(names):
        n = int(fx["frame_len"][i])
        cols = [fx[f"frame_{k}"][i:i + 1, :n] for k in (*tc.INPUTS, "quote_volume", "atr")]
        res = ref.top_gainer_entry(*cols)
        assert res["status"][0, -1] == fx["frame_status"][i], name
        assert res["entry"][0, -3] == fx["frame_entry"][i], name
        want = dict(zip(ref.TGE_KEYS, fx["frame_values"][i]))
        for k in ref.TGE_KEYS:
            g = res["values"][k][0, -3]
            if k in ref.APPROX_KEYS:
                assert np.isnan(g) == np.isnan(want[k]) and (np.isnan(g) or abs(g - want[k]) <= 1e-9 * abs(want[k])), k
            else:
                assert tc.same_bits(np.array([g]), np.array([want[k]])).all(), (name, k)
        for k, f in (("score", "frame_score"), ("stop_loss_pct", "frame_stop")):
            g, w = res[k][0, -1], fx[f][i]
            assert np.isnan(g) == np.isnan(w) and (np.isnan(g) or abs(g - w) <= 1e-9 * abs(w)), (name, k)
        got[name] = ref.TGE_REASONS[int(res["status"][0, -1])]
    assert got["breakout_frame"] == got["short_history_frame"] == "top_gainer_breakout_two_close_confirmation"
    assert got["short_history_extension_cap"] == "extension_move_too_extended"
    assert got["one_hour_move_too_extended"] == "one_hour_move_too_extended"
    assert got["first_confirmation"] == "first_confirmation_did_not_hold_breakout"
    assert got["second_confirmation"] == "second_confirmation_did_not_clear_breakout_close"
    assert got["fifty_seven_rows"] == "history_too_short"


def test_tables_cover_the_fixture():
    from binquant_amd import _lib, engine, signals

    fx = tc.fixture()
    assert [signals.TGE_REASONS[c] for c in range(18)] == [str(r) for r in fx["reasons"]] == list(ref.TGE_REASONS)
    assert signals.TGE_ENTRY_REASONS[0] == str(fx["entry_ok"]) == ref.TGE_ENTRY_OK
    assert [signals.TGE_ENTRY_REASONS[c] for c in range(1, 15)] == list(ref.TGE_REASONS[1:15])
    assert signals.TGE_KEYS == tuple(str(k) for k in fx["keys"]) == ref.TGE_KEYS == _lib.TGE_VALUES == signals.TG_KEYS
    assert signals.TGE_NO_FRAME == ref.TGE_NO_FRAME == _lib.BQ_TGE_NO_FRAME == 255
    assert (signals.TGE_FIRST_CONFIRM, signals.TGE_SECOND_CONFIRM, signals.TGE_RISK_REJECTED) == (15, 16, 17) == (
        _lib.BQ_TGE_FIRST_CONFIRM, _lib.BQ_TGE_SECOND_CONFIRM, _lib.BQ_TGE_RISK_REJECTED)
    assert engine.TOP_GAINER_DEFAULTS == ref.DEFAULTS
    assert signals.TG_RISK_REASONS == tuple(str(r) for r in fx["risk_reasons"]) == ref.TG_RISK_REASONS


def test_risk_restatement_equals_reference():
    fx = tc.fixture()
    cases = pg.risk_cases()
    assert len(cases) == len(fx["risk_reason"]) and len(cases) >= 300
    for k in cases[0]:   # the stored inputs are the regenerated ones
        assert [c[k] if c[k] is not None else "" for c in cases] == fx[f"risk_in_{k}"].tolist(), k
    assert [ref.risk_allows(c) for c in cases] == fx["risk_reason"].tolist()
    assert (np.bincount(fx["risk_reason"], minlength=10) >= 8).all()


@pytest.fixture
def no_library(monkeypatch):
    """The wrappers must raise before the native library is loaded."""
    from binquant_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the native library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(torch.cuda, "is_available", refuse)


def _host_args(S=3, T=80):
    return [torch.ones((S, T), dtype=torch.float64) for _ in range(5)]


def test_wrapper_rejects_bad_arguments(no_library):
    from binquant_amd import engine, signals

    for i in range(5):   # a float32 panel
        a = _host_args()
        a[i] = a[i].float()
        with pytest.raises(ValueError, match="float64"):
            signals.top_gainer_entry(*a)
    a = _host_args()
    a[2] = a[2][:, :-1]   # a column of another shape
    with pytest.raises(ValueError, match="shape"):
        signals.top_gainer_entry(*a)
    with pytest.raises(ValueError, match="quote_volume"):
        signals.top_gainer_entry(*_host_args(), torch.ones((3, 80)))
    with pytest.raises(ValueError, match="atr"):
        signals.top_gainer_entry(*_host_args(), None, torch.ones((3, 79), dtype=torch.float64))
    with pytest.raises(ValueError, match="risk_ok"):
        signals.top_gainer_entry(*_host_args(), risk_ok=torch.ones((3, 80), dtype=torch.uint8))
    with pytest.raises(ValueError, match="lens"):
        signals.top_gainer_entry(*_host_args(), lens=[1, 2])
    with pytest.raises(ValueError, match="first_t"):
        signals.top_gainer_entry(*_host_args(), first_t=torch.zeros(3))
    with pytest.raises(ValueError, match="min_history"):
        signals.top_gainer_entry(*_host_args(), min_history=24)
    for k in ("lookback_high", "volume_window", "full_extension_bars"):
        for bad in (0, 97):
            with pytest.raises(ValueError, match=k):
                signals.top_gainer_entry(*_host_args(), **{k: bad})
    with pytest.raises(ValueError, match="unknown thresholds"):
        signals.top_gainer_entry(*_host_args(), min_volume_ration=2.0)
    with pytest.raises(ValueError, match="unknown columns"):
        engine.top_gainer_entry(*_host_args(), columns=("rsi",))
    with pytest.raises(ValueError, match="CUDA"):   # well-formed host tensors: no CPU path
        signals.top_gainer_entry(*_host_args())


def test_library_rejects_bad_arguments_without_device():
    """bq_top_gainer_entry validates before any HIP call (fake, never
    dereferenced pointers)."""
    import ctypes

    from binquant_amd import _lib

    lib = _lib.load()
    p = _lib.BqTopGainerParams()
    lib.bq_top_gainer_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    x, null = 0x1000, None

    def call(open_=x, volume=x, status=x, entry=x, S=4, T=100, ld=100, ld_out=100, qv=null, ld_qv=100, atr=null,
             ld_atr=100, risk=null, ld_risk=100, params=None):
        return lib.bq_top_gainer_entry(open_, x, x, x, volume, ld, qv, ld_qv, atr, ld_atr, risk, ld_risk, null, null,
                                       S, T, params, status, entry, null, null, None, ld_out, null)

    for kw in (dict(open_=null), dict(volume=null), dict(status=null), dict(entry=null), dict(S=-1), dict(T=-1),
               dict(ld=99), dict(ld_out=99), dict(qv=x, ld_qv=99), dict(atr=x, ld_atr=99), dict(risk=x, ld_risk=99),
               dict(T=2**31 - 100, ld=2**31, ld_out=2**31), dict(S=2**31)):
        assert call(**kw) == _lib.BQ_EINVAL, kw
    for k, bad in (("lookback_high", 97), ("lookback_high", 0), ("volume_window", 97), ("volume_window", 0),
                   ("full_extension_bars", 97), ("full_extension_bars", 0), ("min_history", 24)):
        lib.bq_top_gainer_default_params(ctypes.byref(p))
        setattr(p, k, bad)
        assert call(params=ctypes.byref(p)) == _lib.BQ_EINVAL, (k, bad)
    assert _lib.TGE_MAX_LOOKBACK == 96
    assert call(S=0) == _lib.BQ_OK and call(T=0, ld=0, ld_out=0) == _lib.BQ_OK   # nothing to do: no launch
