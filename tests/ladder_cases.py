"""Shared inputs of tests/test_ladder_ref.py, tests/test_ladder_args.py,
tests/test_ladder_gpu.py and tests/test_ladder_cohort_gpu.py: the fixture
tests/golden/ladder_gates.npz with its regenerated panel, the hand-built cases
for the kernel's tile and 64-slot edges, and the comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import ladder_panel_gen as pg   # noqa: E402
import ladder_ref as ref        # noqa: E402

BB = ("bb_upper", "bb_mid", "bb_lower")
BANDS = ("bb_high", "bb_mid_arg", "bb_low")
RECORDINGS = ("plain", "r6")    # the bands as the frame holds them / rounded to 6 places by the caller


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "ladder_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    """The fixture's inputs in replay()'s argument names (computed once; do not modify)."""
    p = pg.ladder_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "ladder_panel_gen drifted from the recorded inputs"
    sym = dict(ok=p["sym_ok"] & pg.context_ok(p)[None, :], **{k: p[k] for k in ref.SYM_KEYS[1:]})
    return dict(p, ctx_ok=pg.context_ok(p), sym=sym)


@functools.lru_cache(maxsize=1)
def rounded():
    b = pg.rounded_bands(pg.ladder_panel())
    assert pg.digest(b) == str(fixture()["bands_digest"]), "rounded_bands drifted from the recorded inputs"
    return b


@functools.lru_cache(maxsize=1)
def policy_cases():
    c = pg.policy_cases()
    assert pg.digest(c) == str(fixture()["policy_digest"]), "policy_cases drifted from the recorded inputs"
    return c


def bands_of(recording: str):
    """replay()'s `bands` of a recording: None for the frame's own columns."""
    return None if recording == "plain" else tuple(rounded()[k] for k in BANDS)


def recorded(recording: str) -> dict:
    fx = fixture()
    pre = "" if recording == "plain" else "r6."
    out = {k: fx[pre + k] for k in ("status",) + ref.VALUES[1:]}
    out["bb_change_pct"] = fx["bb_change_pct"]   # formed from the frame's columns: one array for both recordings
    return out


def ref_replay(p: dict, **kw):
    return ref.replay(p["close"], *(p[k] for k in BB), p["market_regime"], p["long_regime_score"], p.get("ctx_ok"),
                      p.get("policy_ok"), sym=p.get("sym"), **kw)


@functools.lru_cache(maxsize=2)
def fixture_replay(recording: str):
    """The restatement on the fixture panel (computed once; do not modify)."""
    p = panel()
    return ref_replay(p, bands=bands_of(recording), first_t=p["first_t"], lens=p["lens"])


def same_bits(a, b) -> np.ndarray:
    """Element-wise: both NaN, or the same value with the same sign of zero."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | ((a == b) & (np.signbit(a) == np.signbit(b)))


def assert_codes_equal(got, want, what=""):
    g, w = np.asarray(got["status"]), np.asarray(want["status"])
    assert g.shape == w.shape, f"{what}: status shape {g.shape} != {w.shape}"
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: status differs at {bad[:5].tolist()}: " \
                          f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"


def assert_values_equal(got, want, what="", names=ref.VALUES):
    for name in names:
        bad = np.argwhere(~same_bits(got[name], want[name]))
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(got[name][tuple(i)], want[name][tuple(i)]) for i in bad[:5]]}"


FIRSTS = (0, 5, 63, 64)


def edge_rows(S, T):
    """first_t cycling over 0 / 5 / 63 / 64 (clipped to the panel); the last row of two or more has lens = T - 2."""
    first = np.array([FIRSTS[(s + 1) % 4] if S > 1 else 0 for s in range(S)]).clip(0, max(T - 1, 0))
    lens = np.full(S, T)
    if S > 1:
        lens[S - 1] = max(T - 2, 1)
    return first, lens


def edge_panel(S: int, T: int, seed: int, ctx_T: int | None = None, sym: str = "cell") -> dict:
    """Bands whose width drifts slowly with a few jumps, dense in what the
    kernel can get wrong: scattered rows with bb_mid <= 0, width <= 0 and NaN
    bands, closes on and outside the bands, NaN scores, strengths and ATRs, and
    contexts most of which pass. ctx_T: 1 or T (default T); sym: "cell"
    ([S, T]), "row" ([S]) or "none"."""
    rng = np.random.default_rng(seed)
    mid = 10.0 ** rng.uniform(0.0, 2.0, (S, 1)) * np.exp(np.cumsum(rng.normal(0.0, 0.002, (S, T)), axis=1))
    half = rng.uniform(0.008, 0.04, (S, 1)) * np.exp(np.cumsum(rng.normal(0.0, 0.02, (S, T)), axis=1))
    for s in range(S):
        for t in rng.integers(0, T, max(T // 80, 1)):
            half[s, t:] *= 1.4
    upper, lower = mid * (1.0 + half), mid * (1.0 - half)
    close = mid + rng.uniform(-1.1, 1.1, (S, T)) * (upper - mid)
    u = rng.random((S, T))
    mid[u < 0.01] = 0.0
    mid[(u >= 0.01) & (u < 0.02)] *= -1.0
    swap = (u >= 0.02) & (u < 0.03)
    upper[swap], lower[swap] = lower[swap], upper[swap]
    upper[(u >= 0.03) & (u < 0.035)] = np.nan
    mid[(u >= 0.035) & (u < 0.04)] = np.nan
    lower[(u >= 0.04) & (u < 0.045)] = np.nan
    on = (u >= 0.05) & (u < 0.07)
    close[on] = np.where(rng.random(on.sum()) < 0.5, lower[on], upper[on])
    close[(u >= 0.07) & (u < 0.075)] = np.nan
    Tc = T if ctx_T is None else ctx_T
    mk = rng.choice([-1, 0, 1, 2, 3, 4], Tc, p=[0.03, 0.02, 0.02, 0.89, 0.02, 0.02]).astype(np.int8)
    score = np.where(rng.random(Tc) < 0.9, rng.uniform(0.2, 0.9, Tc), rng.uniform(-0.2, 0.2, Tc))
    score[rng.random(Tc) < 0.05] = np.nan
    if Tc == 1:
        mk[:], score[:] = ref.RANGE, 0.5
    out = dict(close=close, bb_upper=upper, bb_mid=mid, bb_lower=lower, market_regime=mk, long_regime_score=score,
               ctx_ok=rng.random(Tc) < (0.95 if Tc > 1 else 2.0), policy_ok=rng.random(Tc) < (0.95 if Tc > 1 else 2.0))
    if sym == "none":
        return out
    shape = (S, T) if sym == "cell" else (S,)
    rs = np.where(rng.random(shape) < 0.9, rng.uniform(0.001, 0.4, shape), rng.uniform(-0.2, 0.0, shape))
    rs[rng.random(shape) < 0.05] = np.nan
    atr = rng.uniform(0.0005, 0.05, shape)
    atr[rng.random(shape) < 0.05] = np.nan
    trans = np.where(rng.random(shape) < 0.7, ref.NONE, rng.integers(0, len(ref.MICRO_TRANSITIONS), shape))
    micro = np.where(rng.random(shape) < 0.93, ref.RANGE, rng.integers(0, len(ref.MICRO_REGIMES), shape))
    out["sym"] = dict(ok=rng.random(shape) < 0.96, micro_regime=micro.astype(np.uint8),
                      micro_transition=trans.astype(np.uint8), above_ema20=rng.random(shape) < 0.7,
                      above_ema50=rng.random(shape) < 0.7, rs_vs_btc=rs, atr_pct=atr)
    if sym == "row" and S:   # row 0 passes every symbol gate, so that some candles get to the frame's tests
        for k, v in dict(ok=True, micro_regime=ref.RANGE, micro_transition=ref.NONE, above_ema20=True, rs_vs_btc=0.1).items():
            out["sym"][k][0] = v
    return out
