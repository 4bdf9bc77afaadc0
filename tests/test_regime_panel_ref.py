"""The host restatement of the per-symbol regime panel (tests/regime_panel_ref.py)
against the REAL reference's own output (tests/golden/regime_panel.npz,
make_golden_regime_panel.py): fed the reference's feature values, every label
and flag is exact and every strength is bit for bit, with the candle's own
context (get_context) and with the provider's carried one
(latest_market_context)."""

import numpy as np
import pytest

from binquant_amd import _lib
from tests import regime_panel_ref as ref


@pytest.fixture(scope="module")
def fx():
    return ref.fixture()


def test_fixture_covers_what_it_is_for(fx):
    assert tuple(fx["regimes"]) == _lib.MICRO_REGIMES and tuple(fx["transitions"]) == _lib.MICRO_TRANSITIONS
    has = fx["has"]
    assert has.shape == (ref.gen.S, ref.gen.T) and not has[:, ~fx["exists"]].any()
    assert set(np.unique(fx["micro_regime"][has])) == set(range(5))
    assert set(np.unique(fx["micro_transition"][has])) == set(range(-1, 9))
    idx = np.flatnonzero(fx["exists"])
    assert (np.diff(idx) > 1).any()   # a valid context follows a gated stretch: prev is not t - 1
    # symbols with an entry whose predecessor context has none for them
    at, prev = ref.context_columns(fx["exists"], carry=False)
    absent = sum(int((has[:, t] & ~has[:, prev[t]]).sum()) for t in idx if prev[t] >= 0)
    assert absent >= 20
    near = ref.gen.near_cut(fx["trend_score"], fx["above_ema20"], fx["above_ema50"], fx["rs_vs_btc"], fx["bb_width"],
                            fx["atr_pct"], fx["return_pct"])
    assert not near[has].any()
    # the recorded panel is the generator's
    assert (fx["timestamps"] == ref.gen.timestamps()).all()


@pytest.mark.parametrize("carry", [False, True])
def test_restatement_matches_reference(fx, carry):
    has, exists = fx["has"], fx["exists"]
    at, prev = ref.context_columns(exists, carry)
    if carry:   # the provider's rule, as the generator recorded it
        np.testing.assert_array_equal(at, fx["latest"])
    got = ref.annotate_panel(fx["trend_score"], fx["above_ema20"], fx["above_ema50"], fx["rs_vs_btc"], fx["bb_width"],
                             fx["atr_pct"], fx["return_pct"], has, at, prev)
    seen = at >= 0
    j = at[seen]
    want_ok = np.zeros(has.shape, dtype=np.uint8)
    want_ok[:, seen] = has[:, j]
    np.testing.assert_array_equal(got["ok"], want_ok)
    ok = want_ok.astype(bool)
    for name in ("micro_regime", "micro_transition"):
        want = np.full(has.shape, ref.NONE, dtype=np.uint8)
        want[:, seen] = np.where(fx[name][:, j] < 0, ref.NONE, fx[name][:, j]).astype(np.uint8)
        want[~ok] = ref.NONE
        np.testing.assert_array_equal(got[name], want, err_msg=name)
    for name in ("micro_regime_strength", "micro_transition_strength"):
        want = np.full(has.shape, np.nan)
        want[:, seen] = fx[name][:, j]
        # bit for bit: same NaN cells, same bytes elsewhere
        np.testing.assert_array_equal(np.isnan(got[name]), ~ok, err_msg=name)
        assert got[name][ok].tobytes() == want[ok].tobytes(), name
    assert ok.sum() == (has[:, j].sum())   # no cell left out
