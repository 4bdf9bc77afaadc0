"""CPU: the numpy / pandas restatement of RangeBbRsiMeanReversion.signal()
(tests/rangefade_ref.py) equals what the real method did
(tests/golden/rangefade_gates.npz, written by
tests/golden/make_golden_rangefade.py): codes exact, values bit for bit."""

import numpy as np
import pandas as pd

from tests import rangefade_cases as rc
from tests.rangefade_cases import pg, ref


def _replay(**kw):
    p = rc.panel()
    return ref.replay(*(p[k] for k in rc.PANELS), p["ctx"], p["ctx_ok"], sym=pg.sym_of(p), first_t=p["first_t"],
                      lens=p["lens"], **kw)


def test_panel_digest_and_defaults():
    fx = rc.fixture()
    rc.panel()   # asserts the digest
    assert dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist())) == \
        {k: float(v) for k, v in ref.DEFAULTS.items()}
    assert tuple(fx["reasons"].tolist()) == ref.REASONS and tuple(fx["names"].tolist()) == pg.NAMES
    assert fx["status"].shape == (pg.S, pg.T)


def test_library_tables_equal_the_restatement():
    from binquant_amd import _lib, engine, signals

    assert _lib.RF_REASONS == ref.REASONS and _lib.RF_VALUES == ref.VALUES and _lib.RF_CTX_ROWS == ref.CTX_ROWS
    assert engine.RANGE_FADE_DEFAULTS == ref.DEFAULTS and signals.RF_SYM_KEYS == ref.SYM_KEYS
    assert _lib.MARKET_REGIMES == ref.MARKET_REGIMES and _lib.MICRO_REGIMES == ref.MICRO_REGIMES
    assert _lib.MICRO_TRANSITIONS == ref.MICRO_TRANSITIONS and _lib.MR_NONE == ref.NONE
    assert (signals.RF_EMIT, signals.RF_NO_FRAME, signals.RF_NO_SETUP) == (ref.EMIT, ref.NO_FRAME, ref.NO_SETUP)
    assert (signals.RF_LONG, signals.RF_SHORT) == (ref.LONG, ref.SHORT)
    p = _lib.BqRangeFadeParams()
    _lib.load().bq_range_fade_default_params(p)
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS


def test_restatement_equals_the_recording_with_its_own_features():
    fx = rc.fixture()
    got, want = _replay(), rc.recorded()
    rc.assert_codes_equal(got, want, "restatement")
    rc.assert_values_bits(got, want, "restatement")   # pandas' own rolling sums: the method's bits
    emit = fx["status"] == ref.EMIT
    assert (fx["direction"][emit] == ref.LONG).sum() >= 5 and (fx["direction"][emit] == ref.SHORT).sum() >= 5
    for k, first in (("adx", ref.ADX_TOO_HIGH), ("zscore", ref.NO_SETUP)):   # written from that code on
        assert (np.isnan(fx[k]) == ~(emit | (fx["status"] >= first))).all(), k


def test_restatement_equals_the_recording_with_recorded_features():
    got, want = _replay(features_given=rc.recorded_features()), rc.recorded()
    rc.assert_codes_equal(got, want, "restatement, features given")
    rc.assert_values_bits(got, want, "restatement, features given")


def test_every_code_is_recorded():
    counts = np.bincount(rc.fixture()["status"].ravel(), minlength=len(ref.REASONS))
    assert (counts[2:] >= 10).all(), dict(zip(ref.REASONS, counts.tolist()))


def test_adx_warm_up_is_zero_filled():
    """dx is 0.0, not NaN, while the sums are not ready: the 14-bar mean of dx
    is finite from frame row 13 on and includes those zeros; 100 before."""
    rng = np.random.default_rng(3)
    c = pd.Series(100.0 + np.cumsum(rng.normal(0, 0.5, 40)))
    h, l = c + rng.uniform(0.1, 0.6, 40), c - rng.uniform(0.1, 0.6, 40)
    adx = ref.adx_series(h, l, c).to_numpy()
    assert (adx[:13] == 100.0).all() and np.isfinite(adx[13:]).all()
    assert 0.0 < adx[13] < 100.0 / 14 + 1e-12     # one dx of at most 100 among thirteen zeros
    flat = pd.Series(np.full(30, 7.0))
    assert (ref.adx_series(flat, flat, flat).to_numpy()[13:] == 0.0).all()   # a zero true-range sum: dx = 0.0
    assert (ref.zscore_series(flat).to_numpy() == 0.0).all()                  # std exactly 0: z exactly 0.0


def test_from_t_leaves_the_features_alone():
    p = rc.seeded_panel(3, 103, seed=5)
    whole = rc.ref_replay(p)
    part = rc.ref_replay(p, from_t=np.full(3, 70))
    assert (part["status"][:, :70] == ref.NO_FRAME).all()
    assert (part["status"][:, 70:] == whole["status"][:, 70:]).all()
    for k in ref.VALUES:
        assert rc.same_bits(part[k][:, 70:], whole[k][:, 70:]).all(), k
    assert (whole["status"] == ref.EMIT).sum() >= 3
