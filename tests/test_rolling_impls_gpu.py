"""Every kernel behind each rolling statistic gives the same bits: the
register-resident sorted window (on one lane, or split over a lane pair or
quad) vs the per-wave sorted union vs the per-output sorting network (order
statistics), the class-specialised re-staging replay vs the all-classes one
(moments, ewm). Each implementation is forced in its own child process
(BQ_RANK_IMPL / BQ_REPLAY_IMPL / BQ_SLIDE_*) over the same battery — NaN gaps,
constant runs, signed zeros, shifts, min_periods, windows on both sides of
every dispatch boundary — and the order statistics, the moments, the ewm
series and the fill are also checked against pandas, bit for bit."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


def _run(tmp_path, name, env):
    out = tmp_path / f"{name}.npz"
    e = dict(os.environ, **env, PYTHONPATH=str(HERE.parent))
    subprocess.run([sys.executable, str(HERE / "rolling_impl_run.py"), str(out)], env=e, check=True, timeout=240)
    return np.load(out)


def test_rolling_implementations_agree_bitwise(cuda, tmp_path):
    sys.path.insert(0, str(HERE))
    from rolling_impl_run import RANK_JOBS, panel

    runs = {
        "tile_restage": _run(tmp_path, "tile_restage", {"BQ_RANK_IMPL": "tile", "BQ_REPLAY_IMPL": "restage"}),
        "stencil_mixed": _run(tmp_path, "stencil_mixed", {"BQ_RANK_IMPL": "stencil", "BQ_REPLAY_IMPL": "mixed"}),
        "slide": _run(tmp_path, "slide", {"BQ_RANK_IMPL": "slide", "BQ_SLIDE_PAIR_MIN": "0"}),
        "slide_pair": _run(tmp_path, "slide_pair", {"BQ_RANK_IMPL": "slide", "BQ_SLIDE_PAIR_MIN": "48",
                                                    "BQ_SLIDE_GROUP": "2"}),
        "slide_quad": _run(tmp_path, "slide_quad", {"BQ_RANK_IMPL": "slide", "BQ_SLIDE_PAIR_MIN": "48",
                                                    "BQ_SLIDE_GROUP": "4"}),
        "restage": _run(tmp_path, "restage", {"BQ_REPLAY_IMPL": "restage"}),
        "auto": _run(tmp_path, "auto", {}),
    }
    ref = runs["auto"]
    for name, r in runs.items():
        assert set(r.files) == set(ref.files)
        for k in ref.files:
            a, b = r[k], ref[k]
            np.testing.assert_array_equal(a, b, err_msg=f"{name}: {k}")   # NaN == NaN here
            # signs of zero must agree too, except for order statistics: which of
            # -0.0 / +0.0 a window's rank holds is unspecified (they compare
            # equal; pandas' skiplist keeps insertion order)
            if b.dtype == bool:   # crossing flags
                continue
            num = ~np.isnan(b) & ~(k.startswith(("rank", "short", "xthr")) & (b == 0))
            assert np.array_equal(np.signbit(a[num]), np.signbit(b[num])), (name, k)
    # the flags are those of the thresholds (x >= thr) & (x.shift(1) < thr.shift(1))
    xv = panel(37, 700).cpu().numpy()
    for k, (w, q, mp, sh) in zip((0, 1), ((48, 0.8, 48, 1), (80, 0.92, 20, 1))):
        t = ref[f"xthr_{k}"]
        with np.errstate(invalid="ignore"):
            want = (xv >= t) & np.concatenate([np.zeros((37, 1), bool), xv[:, :-1] < t[:, :-1]], axis=1)
        np.testing.assert_array_equal(ref[f"xflag_{k}"], want)
    # order statistics vs pandas on the same battery
    x = panel(37, 700).cpu().numpy()
    df = pd.DataFrame(x.T)
    for w, st, q, mp, sh in RANK_JOBS:
        roll = df.shift(sh).rolling(w, min_periods=mp)
        want = (roll.median() if st == "median" else roll.max() if st == "max" else roll.min() if st == "min"
                else roll.quantile(q, interpolation="lower") if st == "qlower" else roll.quantile(q)).to_numpy().T
        got = ref[f"rank_{w}_{st}_{q}_{mp}_{sh}"]
        np.testing.assert_array_equal(got, want, err_msg=f"w={w} {st} q={q}")
    # moments, ewm and the fill vs pandas on the same battery (the batch's order
    # in rolling_impl_run.main): in one mixed call and one series per call
    wants = [
        df.rolling(2, min_periods=2).sum(),
        df.shift(1).rolling(12, min_periods=12).mean(),
        df.rolling(20, min_periods=20).std(),
        df.rolling(80, min_periods=5).var(ddof=0),
        df.shift(3).rolling(96, min_periods=1).std(ddof=0),
        df.ewm(alpha=1 / 14, adjust=False, min_periods=14).mean(),
        df.ewm(span=50, adjust=False, min_periods=0).mean(),
        df.ffill(),
    ]
    for i, want in enumerate(wants):
        for kind in ("mixed", "single"):
            np.testing.assert_array_equal(ref[f"{kind}_{i}"], want.to_numpy().T, err_msg=f"{kind}_{i}")
    # the mixed batch wider than one grid row of waves
    bdf = pd.DataFrame(panel(5000, 64).cpu().numpy().T)
    for i, want in enumerate([bdf.rolling(3, min_periods=3).sum(), bdf.rolling(10, min_periods=10).std(),
                              bdf.ewm(span=9, adjust=False, min_periods=0).mean()]):
        np.testing.assert_array_equal(ref[f"big_{i}"], want.to_numpy().T, err_msg=f"big_{i}")
