"""The top-gainer breakout gate and two-close confirmation on the device
(signals.top_gainer_entry, bq_topgainer.hip): against the REAL reference's
outputs (tests/golden/topgainer_gates.npz) and, at tile and shape edges,
against the restatement that fixture pins (tests/topgainer_ref.py). Status and
entry exact, point-wise values bit for bit, ema20 / ema50 / the two volume
ratios / score within tests/util's 1e-9; NaN exactly where the contract says."""

import functools

import numpy as np
import pytest
import torch

from tests import topgainer_cases as tc
from tests.topgainer_cases import pg, ref

pytestmark = pytest.mark.gpu

T_EDGES = [1, 57, 58, 59, 1023, 1024, 1025, 1026, 1024 + 96, 2 * 1024 + 5]


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(res):
    return {"status": res["status"].cpu().numpy(), "entry": res["entry"].cpu().numpy(),
            "score": res["score"].cpu().numpy(), "stop_loss_pct": res["stop_loss_pct"].cpu().numpy(),
            "values": {k: v.cpu().numpy() for k, v in res["values"].items()}}


def device_entry(args, **kw):
    from binquant_amd import signals

    for k in ("first_t", "lens"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    if kw.get("risk_ok") is not None:
        kw["risk_ok"] = dv(np.asarray(kw["risk_ok"], bool))
    return host(signals.top_gainer_entry(*(dv(a) for a in args), **kw))


def assert_nan_contract(res, what=""):
    """On every candle: values NaN exactly where the feature status is not
    ready; score NaN exactly off the candidate candles, stop_loss_pct NaN
    there too."""
    ready = (res["entry"] == 0) | ((res["entry"] >= 4) & (res["entry"] <= 14))
    for k, v in res["values"].items():
        assert (np.isnan(v) == ~ready).all(), f"{what}: {k}"
    cand = (res["status"] == 0) | (res["status"] == ref.RISK_REJECTED)
    assert (np.isnan(res["score"]) == ~cand).all(), what
    assert np.isnan(res["stop_loss_pct"][~cand]).all(), what


@pytest.fixture(scope="module")
def panel_runs(cuda):
    """Every recorded run of the fixture panel, one launch each."""
    p = tc.panel()
    out = {}
    for name in tc.RUNS:
        args, kw = tc.run_args(p, name)
        out[name] = device_entry(args, **kw)
    return out


@pytest.mark.parametrize("name", sorted(tc.RUNS))
def test_fixture_panel(panel_runs, name):
    from tests.test_topgainer_ref import recorded, sampled

    fx = tc.fixture()
    res = panel_runs[name]
    tc.assert_entry_equal(sampled(res, fx["positions"], tc.RUNS[name][1]), recorded(fx, name), name)
    assert_nan_contract(res, name)
    assert (res["status"] == 0).sum() >= 50 and (res["status"] == ref.RISK_REJECTED).sum() >= 20


def test_reference_test_frames(cuda):
    """The reference's breakout frame confirms; each mutation its tests apply
    gives its reason string."""
    from binquant_amd import signals

    fx = tc.fixture()
    got = {}
    for i, name in enumerate(str(n) for n in fx["frame_names"]):
        n = int(fx["frame_len"][i])
        res = device_entry([fx[f"frame_{k}"][i:i + 1, :n] for k in (*tc.INPUTS, "quote_volume", "atr")])
        assert res["status"][0, -1] == fx["frame_status"][i] and res["entry"][0, -3] == fx["frame_entry"][i], name
        want = dict(zip(ref.TGE_KEYS, fx["frame_values"][i]))
        for k in ref.TGE_KEYS:
            g = res["values"][k][0, -3:-2]
            if k in ref.APPROX_KEYS:
                tc.assert_close(g, np.array([want[k]]), f"{name}: {k}", scale=abs(np.nan_to_num(want[k])))
            else:
                assert tc.same_bits(g, np.array([want[k]])).all(), (name, k)
        tc.assert_close(res["score"][0, -1:], fx["frame_score"][i:i + 1], f"{name}: score", scale=1.0)
        assert tc.same_bits(res["stop_loss_pct"][0, -1:], fx["frame_stop"][i:i + 1]).all(), name
        got[name] = signals.TGE_REASONS[int(res["status"][0, -1])]
        assert signals.TGE_ENTRY_REASONS[int(res["entry"][0, -3])] == (
            "top_gainer_breakout_ignition" if fx["frame_entry"][i] == 0 else ref.TGE_REASONS[fx["frame_entry"][i]])
    assert got["breakout_frame"] == got["short_history_frame"] == "top_gainer_breakout_two_close_confirmation"
    assert got["short_history_extension_cap"] == "extension_move_too_extended"
    assert got["one_hour_move_too_extended"] == "one_hour_move_too_extended"
    assert got["first_confirmation"] == "first_confirmation_did_not_hold_breakout"
    assert got["second_confirmation"] == "second_confirmation_did_not_clear_breakout_close"
    assert got["fifty_seven_rows"] == "history_too_short"


@functools.lru_cache(maxsize=4)
def edge_panel(S, T):
    return tc.injected_panel(S, T, seed=1000 * S + T)


def check_vs_ref(q, what, qa=True, **kw):
    args = [q[k] for k in tc.INPUTS] + ([q["quote_volume"], q["atr"]] if qa else [None, None])
    want = ref.top_gainer_entry(*args, **kw)
    got = device_entry(args, **kw)
    tc.assert_entry_equal(got, want, what)
    assert_nan_contract(got, what)
    return want


@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("S", [1, 3, 70])
def test_tile_and_shape_edges(cuda, S, T):
    """Breakouts whose confirmation triple, 48-high window, 32-volume window
    and t - 96 anchor straddle tile boundaries; first_t mixed per row; ragged
    lens (0 and < 58 among them); row 2 turns serial after a boundary."""
    q = edge_panel(S, T)
    g = np.random.default_rng(S * 7 + T)
    first = np.where(g.random(S) < 0.5, 0, g.integers(0, max(T - 5, 1), S))
    lens = g.integers(0, T + 1, S)
    lens[0] = T
    if S > 2:
        lens[1], lens[2] = 0, min(T, 40)
    want = check_vs_ref(q, f"{S}x{T}", risk_ok=q["risk_ok"])
    check_vs_ref(q, f"{S}x{T} no qv / atr", qa=False)
    check_vs_ref(q, f"{S}x{T} first_t/lens", first_t=first, lens=lens, risk_ok=q["risk_ok"])
    if S == 70 and T == 2 * 1024 + 5:
        st = want["status"]
        assert (st == 0).sum() >= 30 and len(np.unique(st)) >= 10
        # confirmations whose breakout candle (t - 2) lies in the previous tile
        conf = np.argwhere(st == 0)[:, 1]
        assert np.isin(conf, [1024, 1025]).sum() >= 4 and np.isin(conf, [2048, 2049]).sum() >= 4
        assert np.isnan(q["close"][2, 1025]) and np.isfinite(want["values"]["ema20"][2, 1030:1100]).sum() > 30


def test_padded_row_pitch(cuda):
    """ld = T + 192 input views (the padded enrich outputs) give the
    contiguous call's bits, with the quote volume / ATR on their own pitch too."""
    from binquant_amd import signals

    S, T = 5, 1100
    q = tc.injected_panel(S, T, seed=5)
    names = (*tc.INPUTS, "quote_volume", "atr")
    flat = signals.top_gainer_entry(*(dv(q[k]) for k in names), risk_ok=dv(q["risk_ok"]))

    def padded(a):
        buf = torch.full((S, T + 192), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :T] = dv(a)
        return buf[:, :T]

    cols = [padded(q[k]) for k in names]
    assert cols[0].stride(0) == T + 192
    for mix in (cols, cols[:5] + [dv(q["quote_volume"]), cols[6]], [dv(q[k]) for k in tc.INPUTS] + cols[5:]):
        res = signals.top_gainer_entry(*mix, risk_ok=dv(q["risk_ok"]))
        assert torch.equal(res["status"], flat["status"]) and torch.equal(res["entry"], flat["entry"])
        for k in ("score", "stop_loss_pct"):
            assert torch.equal(res[k].view(torch.int64), flat[k].view(torch.int64)), k
        for k, v in flat["values"].items():
            assert torch.equal(res["values"][k].view(torch.int64), v.view(torch.int64)), k
    assert int((flat["status"] == 0).sum()) >= 5


def test_null_value_columns(cuda):
    """Each value column alone, then none, gives the full call's status and
    that column's bits."""
    from binquant_amd import signals

    q = tc.injected_panel(9, 1100, seed=23)
    args = [dv(q[k]) for k in (*tc.INPUTS, "quote_volume", "atr")]
    full = signals.top_gainer_entry(*args)
    assert tuple(full["values"]) == signals.TGE_KEYS and int((full["status"] == 0).sum()) >= 10
    none = signals.top_gainer_entry(*args, columns=())
    assert none["values"] == {}
    for k in ("status", "entry"):
        assert torch.equal(none[k], full[k])
    for k in ("score", "stop_loss_pct"):
        assert torch.equal(none[k].view(torch.int64), full[k].view(torch.int64))
    for k in signals.TGE_KEYS:
        one = signals.top_gainer_entry(*args, columns=(k,))
        assert list(one["values"]) == [k] and torch.equal(one["status"], full["status"])
        assert torch.equal(one["entry"], full["entry"])
        assert torch.equal(one["values"][k].view(torch.int64), full["values"][k].view(torch.int64)), k


def test_risk_ok_only_turns_confirmations(cuda):
    """risk_ok turns exactly the status-0 candles where it is 0 into
    risk_rejected; every other output is untouched."""
    from binquant_amd import signals

    q = tc.injected_panel(12, 1500, seed=31)
    args = [dv(q[k]) for k in (*tc.INPUTS, "quote_volume", "atr")]
    free = signals.top_gainer_entry(*args)
    risk = dv(q["risk_ok"])
    held = signals.top_gainer_entry(*args, risk_ok=risk)
    turned = (free["status"] == 0) & ~risk
    assert int(turned.sum()) >= 3 and int(((free["status"] == 0) & risk).sum()) >= 10
    want = torch.where(turned, torch.full_like(free["status"], signals.TGE_RISK_REJECTED), free["status"])
    assert torch.equal(held["status"], want) and torch.equal(held["entry"], free["entry"])
    for k in ("score", "stop_loss_pct"):
        assert torch.equal(held[k].view(torch.int64), free[k].view(torch.int64)), k
    for k, v in free["values"].items():
        assert torch.equal(held["values"][k].view(torch.int64), v.view(torch.int64)), k


def test_fused_risk_program(cuda):
    """signals.top_gainer_risk_allows equals the real _risk_profile_allows on
    the fixture's stand-in contexts: one case per candle of a [2, N] panel
    (the context columns broadcast over the symbols)."""
    from binquant_amd import _lib, signals

    fx = tc.fixture()
    cases = pg.risk_cases()
    n = len(cases)
    col = lambda k: torch.tensor([float(c[k]) for c in cases], dtype=torch.float64, device="cuda")   # noqa: E731
    flag = lambda k: torch.tensor([bool(c[k]) for c in cases], device="cuda")                      # noqa: E731
    code = lambda k, names: torch.tensor([names.index(c[k]) if c[k] is not None else -1 for c in cases],   # noqa: E731
                                         dtype=torch.int8, device="cuda")
    wide = lambda x: x.reshape(1, n).expand(2, n).contiguous()   # noqa: E731
    ok, reason = signals.top_gainer_risk_allows(
        col("stress"), col("long_score"), col("short_score"), col("regime_score"), col("btc_return"),
        flag("context_ok"), wide(col("rs")), wide(col("atr_pct")), wide(code("regime", _lib.MICRO_REGIMES)),
        wide(code("transition", _lib.MICRO_TRANSITIONS)), wide(col("trend")), wide(flag("features_ok")))
    assert reason.dtype == torch.uint8 and ok.dtype == torch.bool and tuple(reason.shape) == (2, n)
    for row in range(2):
        assert reason[row].cpu().tolist() == fx["risk_reason"].tolist()
    assert torch.equal(ok, reason == 0)
    assert [signals.TG_RISK_REASONS[c] for c in range(10)] == [str(r) for r in fx["risk_reasons"]]


def _cohort_inputs(S, T, seed):
    from binquant_amd.synth import numpy_panel

    p5 = numpy_panel(S, T, seed0=seed, edges=True)
    q = tc.injected_panel(S, T, seed=seed + 1, nan_rate=0.0)
    ts = np.broadcast_to(pg.T0 + pg.STEP * np.arange(T, dtype=np.int64), (S, T)).copy()
    g = np.random.default_rng(seed + 2)
    btc = 60000.0 * np.exp(np.cumsum(g.normal(0.0, 0.001, T)))
    ins = [dv(p5[k]) for k in ("open", "high", "low", "close", "volume")]
    ins += [dv(q[k]) for k in tc.INPUTS]
    ins += [dv(ts), dv(ts[0]), dv(btc)]
    return ins, dv(q["risk_ok"])


def _same(a, b):
    if a.dtype.is_floating_point:
        return torch.equal(torch.nan_to_num(a, nan=-12345.0), torch.nan_to_num(b, nan=-12345.0))
    return torch.equal(a, b)


def test_cohort_top_entry(cuda):
    """top_entry=True adds exactly the four topentry.* keys, equal to a direct
    call on v15 * c15 and e15.ATR; every other key is bit-equal to the default
    call; captured as a graph and replayed twice it equals eager."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline

    S, T = 64, 400
    (a, risk_a), (b, risk_b) = _cohort_inputs(S, T, 41), _cohort_inputs(S, T, 43)
    plain = process_cohort(*b)
    added = process_cohort(*b, top_entry=True, top_risk=risk_b)
    new = [f"topentry.{k}" for k in ("status", "entry", "score", "stop_loss_pct")]
    assert not any(k.startswith("topentry.") for k in plain)
    assert sorted(k for k in added if k not in plain) == sorted(new)
    assert [k for k in added if k in plain] == list(plain)
    n = int(plain["h1.bins"].max())
    for k in plain:
        x, y = added[k], plain[k]
        if k.startswith("h1.") and x.dim() == 2:   # bins past a row's count are unwritten
            x, y = x[:, :n], y[:, :n]
        assert _same(x, y), k
    o15, h15, l15, c15, v15 = b[5:10]
    direct = signals.top_gainer_entry(o15, h15, l15, c15, v15, v15 * c15, added["e15.ATR"], risk_ok=risk_b)
    for k in ("status", "entry", "score", "stop_loss_pct"):
        assert _same(added[f"topentry.{k}"], direct[k]), k
    assert int((direct["status"] == 0).sum()) >= 10 and int((direct["status"] == 17).sum()) >= 1

    def run(*ins):   # the risk mask travels with the inputs, so a replay reads the new one
        return process_cohort(*ins[:-1], top_entry=True, top_risk=ins[-1])

    graph = CapturedPipeline(run, *a, risk_a)
    for _ in range(2):
        rep = graph(*b, risk_b)
        torch.cuda.synchronize()
        assert list(rep) == list(added)
        for k in added:
            x, y = rep[k], added[k]
            if k.startswith("h1.") and x.dim() == 2:
                x, y = x[:, :n], y[:, :n]
            assert _same(x, y), f"graph {k}"
