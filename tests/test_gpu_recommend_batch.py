"""Batched recommend (cc_recommend_batch_fp32 / Recommender.recommend_many) vs the pinned-order CPU
oracle: every row BIT-EXACT (np.array_equal, no tolerances) and equal to the single-cube path."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes
from oracle import infer_ref, model_ref
from tests import tile_cases

pytestmark = pytest.mark.gpu

SHAPES = [(63, 64), (1001, 128), (4100, 1024)]
_models = {}
_oracle = {}


def limit():
    return int(L.lib().cc_recommend_batch_max_amount())


def model_of(V, d):
    if (V, d) not in _models:
        P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
        _models[(V, d)] = (P, Recommender(Layout(V, d).pack(P), V, d))
    return _models[(V, d)]


def oracle_probs(tag, P, cubes):
    """The oracle's probabilities of every cube, computed once per tag and shared."""
    if tag not in _oracle:
        _oracle[tag] = [infer_ref.recommend_probs(P, c) for c in cubes]
    return _oracle[tag]


def mixed_batch(V):
    """11 rows: n = 0, 1, 32, 33, 65, min(V, 500), V - 1, V (each capped at V); one row unsorted
    with duplicates; two identical rows."""
    rng = np.random.default_rng(V)
    cubes = [rng.choice(V, min(n, V), replace=False) for n in (0, 1, 32, 33, 65, min(V, 500), V - 1, V)]
    base = rng.choice(V, min(V, 40), replace=False)
    cubes.append(rng.permutation(np.concatenate([base, base[:9], base[3:5]])))
    twin = rng.choice(V, min(V, 21), replace=False)
    cubes += [twin, twin.copy()]
    return cubes


def random_cubes(V, R, seed):
    rng = np.random.default_rng(seed)
    return [rng.choice(V, int(rng.integers(0, 201)), replace=False) for _ in range(R)]


def check_row(out, want_p, cube, amount, probs=False):
    adds, _ = infer_ref.top_n(want_p, cube, amount)
    assert out['additions'].dtype == np.int32 and out['add_vals'].dtype == np.float32
    assert out['cut_vals'].dtype == np.float32
    assert np.array_equal(out['additions'], adds)
    assert np.array_equal(out['add_vals'], want_p[adds])
    assert np.array_equal(out['cut_vals'], want_p[np.asarray(cube, np.int64)])
    if probs:
        assert np.array_equal(out['probs'], want_p)


@pytest.mark.parametrize('V,d', SHAPES)
def test_mixed_batch_bit_exact(V, d):
    P, rec = model_of(V, d)
    cubes = mixed_batch(V)
    assert len(cubes) == 11
    want = oracle_probs(('mixed', V, d), P, cubes)
    for amount in (0, 1, 40, limit(), V + 1):           # V + 1 is above every row's V - n
        outs = rec.recommend_many(cubes, amount, want_probs=True)
        assert len(outs) == len(cubes)
        for r, cube in enumerate(cubes):
            check_row(outs[r], want[r], cube, amount, probs=True)
        assert len(outs[7]['additions']) == 0            # n = V: no candidate
        assert len(outs[6]['additions']) == 1            # n = V - 1: one


def _direct(rec, cubes, amount, want_probs=False):
    """cc_recommend_batch_fp32 itself, with the outputs pre-filled with junk."""
    V, d, dev = rec.V, rec.d, rec.dev
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    R, A = len(cubes), max(amount, 1)
    rp = torch.from_numpy(row_ptr).to(dev)
    ix = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(dev)
    ws = torch.full((int(L.lib().cc_recommend_batch_ws_size(V, d, R, max_n)) // 4 + 64,), -1,
                    device=dev, dtype=torch.int32)
    nadd = torch.full((R,), 77, device=dev, dtype=torch.int32)
    adds = torch.full((R, A), 77, device=dev, dtype=torch.int32)
    addv = torch.full((R, A), 7.0, device=dev)
    cutv = torch.full((max(len(idx), 1),), 7.0, device=dev)
    probs = torch.full((R, V), 7.0, device=dev) if want_probs else None
    rc = L.lib().cc_recommend_batch_fp32(L.ptr(rec.params), V, d, R, L.ptr(rp), L.ptr(ix), max_n, amount,
                                         L.ptr(ws), L.ptr(nadd), L.ptr(adds), L.ptr(addv), L.ptr(cutv),
                                         L.ptr(probs), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, row_ptr, idx, nadd.cpu().numpy(), adds.cpu().numpy(), addv.cpu().numpy(), cutv.cpu().numpy()


@pytest.mark.parametrize('V,d', SHAPES)
def test_direct_call_pads_the_tails(V, d):
    P, rec = model_of(V, d)
    cubes = mixed_batch(V)
    want = oracle_probs(('mixed', V, d), P, cubes)
    for amount in (0, 40):
        rc, row_ptr, idx, nadd, adds, addv, cutv = _direct(rec, cubes, amount)
        assert rc == 0
        for r, cube in enumerate(cubes):
            exp, _ = infer_ref.top_n(want[r], cube, amount)
            k = len(exp)
            assert nadd[r] == k == min(max(amount, 1), V - len(np.unique(cube)))
            assert np.array_equal(adds[r, :k], exp) and np.array_equal(addv[r, :k], want[r][exp])
            assert np.all(adds[r, k:] == -1) and np.all(addv[r, k:] == 0.0)
            lo, hi = row_ptr[r], row_ptr[r + 1]
            assert np.array_equal(cutv[lo:hi], want[r][idx[lo:hi]])


def test_row_tile_edges():
    """R = 1, 33, 130 under one launch and under uneven chunks of 32 rows: every row tile height
    (32 / 64 / 128 rows) with a partial last tile."""
    V, d = 1001, 128
    P, rec = model_of(V, d)
    cubes = random_cubes(V, 130, seed=5)
    want = oracle_probs(('random130', V, d), P, cubes)
    for R in (1, 33, 130):
        a = rec.recommend_many(cubes[:R], 40, want_probs=True, rows_per_launch=512)
        b = rec.recommend_many(cubes[:R], 40, want_probs=True, rows_per_launch=32)
        assert len(a) == len(b) == R
        for r in range(R):
            check_row(a[r], want[r], cubes[r], 40, probs=True)
            for key in ('additions', 'add_vals', 'cut_vals', 'probs'):
                assert np.array_equal(a[r][key], b[r][key]), (R, r, key)


@pytest.mark.parametrize('V,d,R', tile_cases.TILE_CASES)
def test_tile_shapes(V, d, R):
    """The output tile's edges (tests/tile_cases.py), one launch of R rows."""
    rec, cubes, want = tile_cases.recommender(V, d), tile_cases.cubes(V, R), tile_cases.probs(V, d, R)
    outs = rec.recommend_many(cubes, 40, want_probs=True)
    assert len(outs) == R
    for r in range(R):
        check_row(outs[r], want[r], cubes[r], 40, probs=True)


def test_ties_at_the_threshold():
    V, d = 1001, 128
    P, _ = model_of(V, d)
    P2 = dict(P)
    P2['decoder/reconstruct/bias'] = np.where(np.arange(V) % 3 == 0, 40.0, -3.0).astype(np.float32)
    rec = Recommender(Layout(V, d).pack(P2), V, d)
    cubes = [np.arange(0, 300, 7), np.zeros(0, np.int64), np.arange(V - 60, V), np.arange(0, V, 3)[5:200]]
    want = oracle_probs(('ties', V, d), P2, cubes)
    assert all(np.sum(w == 1.0) > 100 for w in want)
    for amount in (1, 7, 100):
        outs = rec.recommend_many(cubes, amount)
        for r, cube in enumerate(cubes):
            check_row(outs[r], want[r], cube, amount)
            tie = outs[r]['additions'][outs[r]['add_vals'] == 1.0]
            assert len(tie) == amount                      # the cut falls inside the tie block
            assert np.all(np.diff(tie) < 0)                # equal values: higher card index first


def test_agrees_with_the_single_cube_path():
    V, d = 1001, 128
    _, rec = model_of(V, d)
    cubes = mixed_batch(V)
    for amount in (40, limit() + 1):                       # the second takes the fallback loop
        many = rec.recommend_many(cubes, amount, want_probs=True)
        for r, cube in enumerate(cubes):
            one = rec.recommend(cube, amount, want_probs=True)
            assert sorted(one) == sorted(many[r])
            for key in one:
                assert one[key].dtype == many[r][key].dtype
                assert np.array_equal(one[key], many[r][key]), (amount, r, key)


def test_api_recommend_many_matches_api_recommend():
    from cubecobrarecommender_amd import api
    V, d = 1001, 128
    _, rec = model_of(V, d)

    class Model:
        def recommender(self):
            return rec

    names = {i: f'card {i}' for i in range(V)}
    cubes = [[int(i) for i in c] for c in mixed_batch(V)]
    many = api.recommend_many(Model(), iter(cubes), 40, names)
    assert len(many) == len(cubes)
    for cube, got in zip(cubes, many):
        want = api.recommend(Model(), cube, 40, names)
        assert got == want and list(got['additions']) == list(want['additions'])


def test_row_independence():
    V, d = 1001, 128
    _, rec = model_of(V, d)
    cubes = random_cubes(V, 130, seed=5)
    alone = rec.recommend_many([cubes[77]], 40, want_probs=True)[0]
    among = rec.recommend_many(cubes, 40, want_probs=True)[77]
    for key in alone:
        assert np.array_equal(alone[key], among[key]), key


def test_workspace_state_does_not_leak():
    """The larger batch first: its keys and bitmasks sit beyond the second batch's rows."""
    V, d = 1001, 128
    P, _ = model_of(V, d)
    rec = Recommender(Layout(V, d).pack(P), V, d)
    big, small = random_cubes(V, 130, seed=5), mixed_batch(V)
    want_big = oracle_probs(('random130', V, d), P, big)
    want_small = oracle_probs(('mixed', V, d), P, small)
    for cubes, want in ((big, want_big), (small, want_small)):
        outs = rec.recommend_many(cubes, 40)
        for r, cube in enumerate(cubes):
            check_row(outs[r], want[r], cube, 40)


def test_guards():
    V, d = 63, 64
    _, rec = model_of(V, d)
    rc = _direct(rec, [[1, 2, 3]], limit() + 1)[0]
    assert rc == -1                                        # CC_ERR_ARG
    assert b'amount' in L.lib().cc_last_error_string()
    with pytest.raises(ValueError):
        rec.recommend_many([[1, 2], [3, V]], 5)
    with pytest.raises(ValueError):
        rec.recommend_many([[-1]], 5)
    assert rec.recommend_many([], 5) == []


def test_full_shape():
    V, d = 20884, 512                                      # the reference checkpoint's architecture
    P = model_ref.init_params(V, d, seed=20250301, bias_std=0.01)
    rec = Recommender(Layout(V, d).pack(P), V, d)
    rng = np.random.default_rng(64)
    cubes = [rng.choice(V, int(rng.integers(45, 721)), replace=False) for _ in range(64)]
    outs = rec.recommend_many(cubes, 100, want_probs=True)
    assert len(outs) == 64
    for r in (0, 31, 63):
        check_row(outs[r], infer_ref.recommend_probs(P, cubes[r]), cubes[r], 100, probs=True)
