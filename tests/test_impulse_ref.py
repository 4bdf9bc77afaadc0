"""CPU checks of the impulse-rider / ladder-stability gates: the numpy
restatement (tests/impulse_ref.py) equals what the REAL reference methods
returned (tests/golden/impulse_gates.npz, tests/golden/make_golden_impulse.py)
— status exact, values bit for bit — the reason table covers the fixture's
reasons, and the engine wrappers reject bad arguments before the library is
loaded or a device is touched."""

import numpy as np
import pytest
import torch

from tests import impulse_cases as ic
from tests.impulse_cases import pg, ref


@pytest.mark.parametrize("name", sorted(ic.runs()))
def test_restatement_equals_reference_on_panel(name):
    fx, p = ic.fixture(), ic.panel()
    symbols, b, thresholds = ic.runs()[name]
    rows = np.array(list(symbols))
    pos = fx["positions"][rows]
    values, status = ref.impulse_rider(*(p[k][rows] for k in ("open", "high", "low", "close", "atr", "open_time")),
                                       p[f"bench_{b}_ts"], p[f"bench_{b}_close"], first_t=p["first_t"][rows],
                                       entry_factor=float(fx["entry_factor"]), min_history=int(fx["min_history"]),
                                       **thresholds)
    take = lambda a: np.take_along_axis(a, pos, axis=1)   # noqa: E731
    want = {k: fx[f"{name}_values"][rows][:, :, i] for i, k in enumerate(fx["keys"])}
    ic.assert_gate_equal({k: take(v) for k, v in values.items()}, take(status), want, fx[f"{name}_status"][rows], name)


def test_fixture_holds_every_rejection():
    fx = ic.fixture()
    counts = np.bincount(np.r_[fx["a_A_status"].ravel(), fx["a_B_status"][:16].ravel()], minlength=256)
    assert all(counts[c] >= 3 for c in range(15)), counts[:15]
    assert counts[0] >= 40
    assert [float(x) for x in fx["defaults"]] == [ref.DEFAULTS[k] for k in fx["default_names"]]
    assert float(fx["entry_factor"]) == ref.DEFAULTS["entry_factor"] and int(fx["min_history"]) == 20


def test_restatement_equals_reference_on_frames():
    """The reference test's 20-row frame (entry limit 108.9), its four
    mutations, and the hand-built benchmark frames (fewer than 5 rows, the
    match at position 3 / 4, a duplicated time)."""
    fx = ic.fixture()
    names = [str(n) for n in fx["frame_names"]]
    for i, name in enumerate(names):
        nb = int(fx["frame_nb"][i])
        row = lambda k: fx[f"frame_{k}"][i:i + 1]   # noqa: E731
        values, status = ref.impulse_rider(row("open"), row("high"), row("low"), row("close"), row("atr"),
                                           row("open_time"), fx["frame_bench_ts"][i, :nb],
                                           fx["frame_bench_close"][i, :nb])
        assert status[0, -1] == fx["frame_status"][i], name
        got = np.array([values[k][0, -1] for k in ref.IR_KEYS])
        assert ic.same_bits(got, fx["frame_values"][i]).all(), name
    st = dict(zip(names, (ref.IR_REASONS[c] for c in fx["frame_status"])))
    assert st["reference_frame"] == "relative_strength_impulse_confirmed"
    assert fx["frame_values"][0][ref.IR_KEYS.index("entry_limit_price")] == pytest.approx(108.9)
    for reason in ("impulse_did_not_cross_threshold", "btc_return_too_high",
                   "confirmation_did_not_hold_trigger_close", "atr_pct_too_high"):
        assert st[f"mutation_{reason}"] == reason
    assert st["btc_four_rows"] == st["btc_match_at_3"] == "btc_return_unavailable"
    assert st["btc_match_at_4"] == "relative_strength_impulse_confirmed"
    assert st["btc_dup_later_high"] == "btc_return_too_high"
    assert st["btc_dup_later_flat"] == "relative_strength_impulse_confirmed"


@pytest.mark.parametrize("n,max_change", [(8, 20.0), (3, 5.0)])
def test_bb_restatement_equals_reference(n, max_change):
    fx = ic.fixture()
    stable, change = ref.bb_stable(fx["bb_upper"], fx["bb_mid"], fx["bb_lower"], n, max_change,
                                   first_t=fx["bb_first_t"])
    np.testing.assert_array_equal(stable, fx[f"bb_stable_{n}"])
    assert ic.same_bits(change, fx[f"bb_change_{n}"]).all()
    assert stable.sum() >= 200 and (~stable & ~np.isnan(change)).sum() >= 200


def test_reason_table_covers_the_fixture():
    from binquant_amd import _lib, signals

    fx = ic.fixture()
    assert set(signals.IR_REASONS.values()) == {str(r) for r in fx["seen_reasons"]}
    assert [signals.IR_REASONS[c] for c in range(15)] == [str(r) for r in fx["reasons"]] == list(ref.IR_REASONS)
    assert signals.IR_KEYS == tuple(str(k) for k in fx["keys"]) == ref.IR_KEYS == _lib.IMPULSE_VALUES
    assert signals.IR_NO_FRAME == ref.IR_NO_FRAME == 255 and signals.IR_CONFIRMED == 0
    assert signals.IR_CLOSE_NOT_NEAR_HIGH == _lib.BQ_IR_CLOSE_NOT_NEAR_HIGH == 14
    from binquant_amd import engine

    assert {k: engine.IMPULSE_DEFAULTS[k] for k in ref.DEFAULTS} == ref.DEFAULTS


@pytest.fixture
def no_library(monkeypatch):
    """The wrappers must raise before the native library is loaded."""
    from binquant_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the native library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(torch.cuda, "is_available", refuse)


def _host_args(S=3, T=30):
    f = lambda: torch.ones((S, T), dtype=torch.float64)   # noqa: E731
    ts = (ic.T0 + ic.STEP * torch.arange(T, dtype=torch.int64)).expand(S, T).contiguous()
    return [f(), f(), f(), f(), f(), ts, ts[0].clone(), torch.ones(T, dtype=torch.float64)]


def test_impulse_wrapper_rejects_bad_arguments(no_library):
    from binquant_amd import engine, signals

    for i in range(5):   # a float32 panel
        a = _host_args()
        a[i] = a[i].float()
        with pytest.raises(ValueError, match="float64"):
            engine.impulse_rider(*a)
    a = _host_args()
    a[2] = a[2][:, :-1]   # a column of another shape
    with pytest.raises(ValueError, match="shape"):
        engine.impulse_rider(*a)
    a = _host_args()
    a[5] = a[5].double()   # open_time not int64
    with pytest.raises(ValueError, match="open_time"):
        engine.impulse_rider(*a)
    a = _host_args()
    a[5] = a[5][:2]
    with pytest.raises(ValueError, match="open_time"):
        engine.impulse_rider(*a)
    a = _host_args()
    a[7] = a[7][:-1]   # benchmark columns of different lengths
    with pytest.raises(ValueError, match="bench_close"):
        engine.impulse_rider(*a)
    a = _host_args()
    a[6] = a[6].flip(0)   # a descending benchmark
    with pytest.raises(ValueError, match="ascending"):
        signals.impulse_rider_features(*a)
    with pytest.raises(ValueError, match="lens"):
        engine.impulse_rider(*_host_args(), lens=[1, 2])
    with pytest.raises(ValueError, match="first_t"):
        engine.impulse_rider(*_host_args(), first_t=torch.zeros(3))
    with pytest.raises(ValueError, match="min_history"):
        engine.impulse_rider(*_host_args(), min_history=6)
    with pytest.raises(ValueError, match="unknown thresholds"):
        engine.impulse_rider(*_host_args(), min_impulze=0.1)
    with pytest.raises(ValueError, match="unknown columns"):
        engine.impulse_rider(*_host_args(), columns=("atr",))
    with pytest.raises(ValueError, match="CUDA"):   # well-formed host tensors: no CPU path
        engine.impulse_rider(*_host_args())


def test_bb_stable_wrapper_rejects_bad_arguments(no_library):
    from binquant_amd import engine, signals

    f = lambda: torch.ones((3, 30), dtype=torch.float64)   # noqa: E731
    with pytest.raises(ValueError, match="float64"):
        engine.bb_stable(f(), f().float(), f())
    with pytest.raises(ValueError, match="shape"):
        engine.bb_stable(f(), f(), f()[:2])
    for n in (0, 65):
        with pytest.raises(ValueError, match="n must be"):
            signals.bb_width_stable(f(), f(), f(), n=n)
    with pytest.raises(ValueError, match="lens"):
        engine.bb_stable(f(), f(), f(), lens=[30])
    with pytest.raises(ValueError, match="CUDA"):
        engine.bb_stable(f(), f(), f())


def test_library_rejects_bad_arguments_without_device():
    """bq_impulse_rider / bq_bb_stable validate before any HIP call (fake,
    never dereferenced pointers)."""
    import ctypes

    from binquant_amd import _lib

    lib = _lib.load()
    p = _lib.BqImpulseParams()
    lib.bq_impulse_default_params(ctypes.byref(p))
    assert (p.min_impulse, p.max_impulse, p.min_rs, p.max_btc_return, p.min_conf_return, p.min_close_location,
            p.max_atr_pct, p.entry_factor, p.min_history) == tuple(
        ref.DEFAULTS[k] for k in ("min_impulse", "max_impulse", "min_rs", "max_btc_return", "min_conf_return",
                                  "min_close_location", "max_atr_pct", "entry_factor", "min_history"))
    x, null = 0x1000, None

    def rider(open_=x, status=x, S=4, T=100, ld=100, nb=10, bts=x, params=None):
        return lib.bq_impulse_rider(open_, x, x, x, ld, x, 100, x, 100, null, null, S, T, bts, x, nb, params, status,
                                    None, 100, null)

    assert rider(open_=null) == _lib.BQ_EINVAL
    assert rider(status=null) == _lib.BQ_EINVAL
    assert rider(S=-1) == _lib.BQ_EINVAL
    assert rider(T=-1) == _lib.BQ_EINVAL
    assert rider(ld=99) == _lib.BQ_EINVAL
    assert rider(bts=null) == _lib.BQ_EINVAL          # nb > 0 needs the benchmark frame
    p.min_history = 6
    assert rider(params=ctypes.byref(p)) == _lib.BQ_EINVAL
    assert rider(S=0) == _lib.BQ_OK                   # nothing to do: no launch

    def stable(mid=x, n=8, S=4, T=100, ld=100):
        return lib.bq_bb_stable(x, mid, x, ld, null, null, S, T, n, 20.0, x, null, 100, null)

    assert stable(mid=null) == _lib.BQ_EINVAL
    assert stable(n=0) == _lib.BQ_EINVAL and stable(n=65) == _lib.BQ_EINVAL
    assert stable(ld=99) == _lib.BQ_EINVAL and stable(S=-1) == _lib.BQ_EINVAL
    assert stable(T=0) == _lib.BQ_OK
