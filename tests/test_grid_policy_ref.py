"""CPU: the numpy restatement of GridOnlyPolicy.resolve after _breadth_pair
(tests/ladder_ref.grid_only_policy) reproduces what the real method answered
over the recorded table of (context, regime, previous, latest) cases
(tests/golden/ladder_gates.npz). signals.grid_only_policy is a fused program
and needs a device: it is held to the same table in tests/test_ladder_gpu.py."""

import numpy as np

from tests import ladder_cases as lc
from tests.ladder_cases import ref


def test_policy_restatement_reproduces_the_real_method():
    fx, c = lc.fixture(), lc.policy_cases()
    allow, reason, points = ref.grid_only_policy(c["context_ok"], c["market_regime"], c["previous"], c["latest"])
    assert np.array_equal(allow, fx["policy_allow"])
    assert np.array_equal(reason, fx["policy_reason"])
    assert lc.same_bits(points, fx["policy_points"]).all()
    assert len(np.unique(fx["policy_reason"])) == len(ref.POLICY_REASONS)
    assert (np.isnan(points) == ~allow).all()


def test_reason_names_are_the_methods():
    from binquant_amd import _lib, signals

    assert signals.GRID_POLICY_REASONS == ref.POLICY_REASONS == tuple(lc.fixture()["policy_reasons"])
    assert signals.GRID_ONLY_REGIMES == ref.GRID_ONLY_REGIMES
    assert _lib.MARKET_REGIMES == ref.MARKET_REGIMES
