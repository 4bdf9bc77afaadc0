"""Host side of the fresh context build (no GPU): score_contexts with a
per-timestamp tracked count (symbols list over time: the reference's
len(get_tracked_symbols()) at each refresh,
live_market_context_accumulator.py:96-102, :196-204), the unchanged scalar
form, and the one-collective all-reduce whose column 9 carries the
per-timestamp count."""

import os
import socket
from math import ceil

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from binquant_amd.market_regime.regime import score_contexts


def _partials(T, seed, lo=20, hi=90):
    g = np.random.default_rng(seed)
    P = np.zeros((T, 10))
    n = g.integers(lo, hi, T).astype(float)
    n[0] = 0.0   # a timestamp without any features
    adv = np.floor(n * g.uniform(0, 1, T))
    dec = np.floor((n - adv) * g.uniform(0, 1, T))
    P[:, 0], P[:, 1], P[:, 2] = n, adv, dec
    P[:, 3] = np.floor(n * g.uniform(0, 1, T))
    P[:, 4] = np.floor(n * g.uniform(0, 1, T))
    P[:, 5] = g.normal(0, 0.01, T) * n
    P[:, 6] = g.normal(0, 0.01, T) * n
    P[:, 7] = g.uniform(0.005, 0.05, T) * n
    P[:, 8] = g.uniform(0.02, 0.2, T) * n
    btc_valid = g.random(T) > 0.1
    return P, g.normal(0, 0.01, T), g.normal(0, 0.01, T), btc_valid


def _same(a, b, key):
    """exact equality of every number; NaN matches NaN (its sign bit carries nothing)"""
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=key)


def test_array_total_tracked_equals_scalar_loop():
    T = 200
    P, br, bt, bv = _partials(T, 11)
    tracked = np.random.default_rng(12).integers(0, 120, T)
    tracked[5] = 0
    ts = np.arange(T) * 900_000
    got = score_contexts(P, br, bt, bv, total_tracked=tracked, timestamps=ts)
    assert got.valid.any() and not got.valid.all()
    for t in range(T):
        one = score_contexts(P[t:t + 1], br[t:t + 1], bt[t:t + 1], bv[t:t + 1], total_tracked=int(tracked[t]),
                             timestamps=ts[t:t + 1])
        assert bool(one.valid[0]) == bool(got.valid[t]), t
        for k, v in one.fields.items():
            _same(got.fields[k][t:t + 1], v, f"{k}@{t}")
    # a list works as well as an array; a wrong length is rejected
    again = score_contexts(P, br, bt, bv, total_tracked=tracked.tolist(), timestamps=ts)
    np.testing.assert_array_equal(again.valid, got.valid)
    try:
        score_contexts(P, br, bt, bv, total_tracked=tracked[:-1])
    except ValueError:
        pass
    else:
        raise AssertionError("a total_tracked of the wrong length was accepted")


def _clamp(x, lo=-1.0, hi=1.0):
    return max(lo, min(hi, x))


def test_scalar_total_tracked_bits_from_the_formula():
    """the int form, against _build_context's formulas (:96-204) written out
    here in Python floats — not against saved outputs of score_contexts"""
    T = 150
    P, br, bt, bv = _partials(T, 21)
    for tracked in (0, 30, 57, 100):
        got = score_contexts(P, br, bt, bv, total_tracked=tracked)
        required = max(40, ceil(tracked * 0.7))
        for t in range(T):
            n, adv, dec, a20, a50, sret, strend, satr, sbbw = (float(x) for x in P[t, :9])
            tot = max(float(tracked), n)
            cov = n / tot if tot > 0 else 0.0
            valid = tracked >= required and tracked > 0 and n >= required and n >= 40 and cov >= 0.7
            assert bool(got.valid[t]) == valid, (tracked, t)
            f = got.fields
            assert f["total_tracked_symbols"][t] == int(tot)
            _same(f["coverage_ratio"][t], cov, "coverage_ratio")
            if n == 0:
                continue
            avg_ret = sret / n
            btc_ret = float(br[t]) if bv[t] else 0.0
            btc_score = _clamp(float(br[t]) * 12.0 + float(bt[t]) * 6.0) if bv[t] else 0.0
            stress = (0.4 * _clamp((satr / n - 0.02) * 12.0, 0.0, 1.0) + 0.25 * _clamp((sbbw / n - 0.08) * 4.0, 0.0, 1.0)
                      + 0.35 * _clamp((-avg_ret) * 16.0, 0.0, 1.0))
            breadth = _clamp((adv / n - dec / n) * 1.5)
            ema = _clamp(((a20 / n + a50 / n) - 1.0) * 1.5)
            long_tw = _clamp(0.4 * breadth + 0.2 * ema + 0.25 * btc_score + 0.15 * _clamp(avg_ret * 12.0)
                             - 0.35 * stress)
            short_tw = _clamp(-0.35 * breadth - 0.15 * ema - 0.2 * btc_score - 0.15 * _clamp(avg_ret * 12.0)
                              + 0.45 * stress)
            rs = (sret - n * btc_ret) / n if bv[t] else 0.0
            for k, want in (("average_return", avg_ret), ("market_stress_score", stress), ("long_tailwind", long_tw),
                            ("short_tailwind", short_tw), ("btc_regime_score", btc_score),
                            ("average_relative_strength_vs_btc", rs), ("average_trend_score", strend / n)):
                _same(f[k][t], want, f"{k}@{t} tracked={tracked}")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_partial(rank):
    g = np.random.default_rng(100 + rank)
    P = g.normal(0, 1, (7, 10))
    P[:, 9] = g.integers(0, 50, 7)   # the kernel's per-timestamp tracked count of this shard
    return P


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from binquant_amd.market_regime.batch import reduce_partials

        part = torch.from_numpy(_shard_partial(rank))
        calls = []
        orig = dist.all_reduce

        def counting(*a, **k):
            calls.append(1)
            return orig(*a, **k)

        dist.all_reduce = counting
        try:
            red, tracked = reduce_partials(part, 999, tracked_per_timestamp=True)
        finally:
            dist.all_reduce = orig
        q.put((rank, len(calls), red.numpy().copy(), np.asarray(tracked)))
    finally:
        dist.destroy_process_group()


def test_two_rank_reduce_sums_tracked_column_in_one_collective():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _shard_partial(0) + _shard_partial(1)
    for rank, calls, red, tracked in res:
        assert calls == 1, (rank, calls)
        np.testing.assert_array_equal(red, want)
        assert tracked.dtype == np.int64
        np.testing.assert_array_equal(tracked, want[:, 9].astype(np.int64))


def test_reduce_partials_single_process_keeps_kernel_column():
    from binquant_amd.market_regime.batch import reduce_partials

    P = torch.from_numpy(_shard_partial(3))
    red, tracked = reduce_partials(P.clone(), 999, tracked_per_timestamp=True)
    np.testing.assert_array_equal(red.numpy(), P.numpy())
    np.testing.assert_array_equal(tracked, P[:, 9].numpy().astype(np.int64))
    red, n = reduce_partials(P.clone(), 12)   # the default: column 9 = n_local, an int back
    assert n == 12 and (red[:, 9] == 12.0).all()
