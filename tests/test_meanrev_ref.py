"""CPU: the numpy / pandas restatement of MeanReversionFade.signal()
(tests/meanrev_ref.py) equals what the real method did
(tests/golden/meanrev_gates.npz, written by tests/golden/make_golden_meanrev.py):
codes, state and repeated messages exact, values bit for bit."""

import numpy as np
import pandas as pd

from tests import meanrev_cases as mc
from tests.meanrev_cases import pg, ref


def _replay(**kw):
    p = mc.panel()
    return ref.replay(*(p[k] for k in mc.PANELS), p["open_time"], p["ctx"], **kw)


def test_panel_digest_and_defaults():
    fx = mc.fixture()
    mc.panel()   # asserts the digest
    assert dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist())) == {k: float(v) for k, v in ref.DEFAULTS.items()}
    assert tuple(fx["reasons"].tolist()) == ref.REASONS and tuple(fx["names"].tolist()) == pg.NAMES
    assert fx["status"].shape == (pg.S, pg.T)


def test_restatement_equals_the_recording_with_its_own_features():
    fx = mc.fixture()
    got = _replay(**mc.fixture_kwargs(False))
    want = mc.recorded()
    mc.assert_codes_equal(got, want, "restatement")
    mc.assert_values_bits(got, want, "restatement")   # pandas' own ewm / rolling: the method's bits
    mc.assert_state_equal(got["state"], (fx["state_has"][:, -1], fx["state_last"][:, -1]), "final state")
    rounded = np.round(got["score"], 4)   # _score's round(.., 4)
    emit = fx["status"] == ref.EMIT
    assert emit.sum() >= 10 and (rounded[emit] == fx["score_rounded"][emit]).all()
    assert np.isnan(fx["score_rounded"][~emit]).all()


def test_restatement_equals_the_recording_with_recorded_features():
    got = _replay(**mc.fixture_kwargs(True))
    want = mc.recorded()
    mc.assert_codes_equal(got, want, "restatement, features given")
    mc.assert_values_bits(got, want, "restatement, features given")


def test_state_after_every_candle():
    """The row's strategy_cooldowns entry after candle t = the last emit up to t."""
    fx, p = mc.fixture(), mc.panel()
    for t in (0, 63, 64, 65, 130, pg.T - 1):
        got = _replay(**{**mc.fixture_kwargs(True), "lens": np.minimum(p["lens"], t + 1)})
        mc.assert_state_equal(got["state"], (fx["state_has"][:, t], fx["state_last"][:, t]), f"after candle {t}")


def test_repeated_messages():
    """The same candle sent again, from the entries as they stood after its
    first message: an emitted candle is held, another one answers as before."""
    fx, p = mc.fixture(), mc.panel()
    reps = fx["repeats"]
    assert (fx["repeat_status"] == ref.ALREADY_EMITTED).sum() >= 3
    for i, (s, t) in enumerate(reps):
        s, t = int(s), int(t)
        sub = {k: v[s:s + 1] for k, v in p.items() if isinstance(v, np.ndarray) and v.shape[:1] == (pg.S,)}
        sym = {k: v[s:s + 1] for k, v in pg.sym_of(p).items()}
        ft = {k: v[s:s + 1] for k, v in mc.recorded_features().items()}
        got = ref.replay(*(sub[k] for k in mc.PANELS), sub["open_time"], p["ctx"], p["ctx_ok"], sym=sym,
                         features_given=ft, state=(fx["state_has"][s:s + 1, t], fx["state_last"][s:s + 1, t]),
                         first_t=sub["first_t"], lens=[t + 1], from_t=[t])
        assert got["status"][0, t] == fx["repeat_status"][i], (s, t)
        assert got["state"][1][0] == fx["repeat_last"][i], (s, t)
        assert (np.delete(got["status"][0], t) == ref.NO_FRAME).all()


def test_reference_regressions_hold():
    """tests/test_mean_reversion_fade.py's two pins of the helpers: _rsi of a
    20-bar monotone rally is exactly 100 from row 14 on (NaN before), and
    _trend_score of a flat series is 0."""
    rsi = ref.rsi_series(pd.Series(np.arange(100.0, 120.0)))
    assert rsi.iloc[:14].isna().all() and (rsi.iloc[14:] == 100.0).all()
    flat = np.full((1, 60), 100.0)
    ft = ref.features(flat, np.ones((1, 60)), np.ones((1, 60)))
    assert (ft["trend_score"] == 0.0).all()
    assert (ft["rsi"][0, 14:] == 50.0).all() and np.isnan(ft["rsi"][0, :14]).all()   # no gains, no losses


def test_entry_is_dropped_by_an_earlier_emit_of_the_same_call():
    """A state that holds candle u's open time does not hold u once an
    earlier candle of the same replay has emitted: the entry moved."""
    S, T = 5, 130
    p = mc.seeded_panel(S, T, seed=4)
    base = mc.ref_replay(p, max_trend_score=mc.TREND_CEILING)
    row = int(np.argmax((base["status"] == ref.EMIT).sum(axis=1)))
    emits = np.nonzero(base["status"][row] == ref.EMIT)[0]
    assert len(emits) >= 2
    a, b = int(emits[0]), int(emits[1])
    has, last = np.zeros(S, bool), np.zeros(S, np.int64)
    has[row], last[row] = True, p["open_time"][row, b]
    whole = mc.ref_replay(p, max_trend_score=mc.TREND_CEILING, state=(has, last))
    assert whole["status"][row, a] == ref.EMIT and whole["status"][row, b] == ref.EMIT
    alone = mc.ref_replay(p, max_trend_score=mc.TREND_CEILING, state=(has, last), from_t=np.full(S, b))
    assert alone["status"][row, b] == ref.ALREADY_EMITTED
