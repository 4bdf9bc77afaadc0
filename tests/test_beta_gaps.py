"""a11 on closes with missing (NaN) and zero candles: the oracle's
beta_corr_prefix against the reference's own values on every prefix
(tests/golden/beta_corr_gaps.npz, make_golden_beta_gaps.py) and against
beta_corr_series on closes without gaps. The device side is
tests/test_beta_gaps_gpu.py."""

from pathlib import Path

import numpy as np
import pytest

from oracle import indicators_ref as ref

G = Path(__file__).resolve().parent / "golden"
GAP_CASES = ("gap_alt", "late_listing", "long_gap", "gap_btc", "zero_close", "flat_gap", "sparse")
W = 50


def gap_case(case):
    z = np.load(G / "beta_corr_gaps.npz")
    return tuple(z[f"{case}__{k}"] for k in ("close", "btc", "beta_last", "corr_last"))


def valid_pairs(c, b):
    """Candles that hold a (symbol, benchmark) return pair the reference keeps."""
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = np.log(c[1:] / c[:-1]), np.log(b[1:] / b[:-1])
    return np.r_[False, ~np.isnan(x) & ~np.isnan(y)]


@pytest.mark.parametrize("case", GAP_CASES)
def test_prefix_oracle_matches_reference_golden(case):
    c, b, want_b, want_c = gap_case(case)
    assert c.size <= 420 and c.size == b.size == want_b.size == want_c.size
    beta, corr = ref.beta_corr_prefix(c, b, W)
    assert np.isnan(beta[0]) and np.isnan(corr[0]) and np.isnan(want_b[0]) and np.isnan(want_c[0])
    np.testing.assert_allclose(np.nan_to_num(beta)[1:], want_b[1:], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(np.nan_to_num(corr)[1:], want_c[1:], rtol=1e-12, atol=1e-15)
    # NaN until the window-th valid pair, and never forward-filled over it
    k = np.cumsum(valid_pairs(c, b))
    assert np.isnan(beta[k < W]).all() and np.isnan(corr[k < W]).all()
    assert (want_b[1:][k[1:] < W] == 0.0).all() and (want_c[1:][k[1:] < W] == 0.0).all()


def test_gap_cases_hold_what_they_claim():
    nan_at = lambda v: np.flatnonzero(np.isnan(v)).tolist()  # noqa: E731
    c, b, wb, wc = gap_case("gap_alt")
    assert nan_at(c) == [200, 300, 301, 302, c.size - 1] and not nan_at(b)
    # the last close is missing: the reference answers with the last valid pair
    assert wb[-1] == wb[-2] != 0.0 and wc[-1] == wc[-2] != 0.0
    # 200 takes the returns of 200 and 201: the windows differ from the positional ones
    assert (wb[50:] != 0.0).all()

    c, b, wb, wc = gap_case("late_listing")
    assert nan_at(c) == list(range(120)) and not nan_at(b)
    # the first return is at 121: 50 pairs at candle 170, not at 120 + 50 - 1
    assert (wb[:170][1:] == 0.0).all() and (wb[170:] != 0.0).all()

    c, b, wb, wc = gap_case("long_gap")
    assert nan_at(c) == list(range(150, 220)) and not nan_at(b)
    assert (wb[150:221] == wb[149]).all() and wb[149] != 0.0 and (wb[50:] != 0.0).all()

    c, b, wb, wc = gap_case("gap_btc")
    assert nan_at(b) == [180, 181] and nan_at(c) == [181, 250]
    assert (wb[180:183] == wb[179]).all() and (wb[250:252] == wb[249]).all()

    c, b, wb, wc = gap_case("zero_close")
    assert not nan_at(c) and not nan_at(b) and np.flatnonzero(c == 0.0).tolist() == [260]
    beta, corr = ref.beta_corr_prefix(c, b, W)
    # -inf at 260, +inf at 261: every window holding either is NaN (51
    # candles), NaN in the oracle and not a computed 0; then the values recover
    assert np.flatnonzero(np.isnan(beta[W:])).tolist() == (np.arange(260, 311) - W).tolist()
    assert np.flatnonzero(np.isnan(corr[W:])).tolist() == (np.arange(260, 311) - W).tolist()
    assert (wb[260:311] == 0.0).all() and (wb[311:] != 0.0).all() and (wb[W:260] != 0.0).all()

    c, b, wb, wc = gap_case("flat_gap")
    assert nan_at(c) == [230] and (c[200:230] == c[200]).all() and (c[231:261] == c[200]).all()
    beta, corr = ref.beta_corr_prefix(c, b, W)
    # 58 zero returns (201-229, 232-260) around two dropped pairs: the windows
    # ending at 252-260 hold equal values only: exact 0 covariance, NaN corr
    flat = np.arange(252, 261)
    assert (beta[flat] == 0.0).all() and np.isnan(corr[flat]).all()
    assert (wb[flat] == 0.0).all() and (wc[flat] == 0.0).all()
    assert not np.isnan(corr[[251, 261]]).any()

    c, b, wb, wc = gap_case("sparse")
    assert c.size == 120 and nan_at(c) == list(range(0, 120, 3))
    assert valid_pairs(c, b).sum() < W
    assert (wb[1:] == 0.0).all() and (wc[1:] == 0.0).all()
    beta, corr = ref.beta_corr_prefix(c, b, W)
    assert np.isnan(beta).all() and np.isnan(corr).all()


@pytest.mark.parametrize("case", ("corr_pos", "corr_neg", "short"))
@pytest.mark.parametrize("window", (5, 50))
def test_prefix_oracle_equals_series_oracle_without_gaps(case, window):
    z = np.load(G / "beta_corr.npz")
    c, b = z[f"{case}__close"], z[f"{case}__btc"]
    beta, corr = ref.beta_corr_prefix(c, b, window)
    wb, wc = ref.beta_corr_series(c, b, window)
    np.testing.assert_array_equal(beta, wb)
    np.testing.assert_array_equal(corr, wc)
