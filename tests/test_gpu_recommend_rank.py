"""Batched recommend above cc_recommend_batch_max_amount(): cc_recommend_batch_rank_fp32 ranks every
card of every row on the device.  Every row is BIT-EXACT (np.array_equal, no tolerances) against the
pinned-order CPU oracle and equal to the single-cube path."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes
from oracle import infer_ref, model_ref
from oracle.detmath import det_sigmoid32
from tests import tile_cases

pytestmark = pytest.mark.gpu

# V below one wave slice; fewer items than threads; several items per thread, V no multiple of 64
# or 1024 and V - n > 2048
SHAPES = [(63, 64), (1001, 128), (4100, 128)]
ALL = 30000                                            # the web endpoint's default: above every V
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


def _direct(rec, cubes, amount, want_probs=False, R=None, ws_shift=0, max_n=None, null=False):
    """cc_recommend_batch_rank_fp32 itself, with the outputs pre-filled with junk."""
    V, d, dev = rec.V, rec.d, rec.dev
    row_ptr, idx, mn, _, _ = pack_cubes(cubes, V)
    max_n = mn if max_n is None else max_n
    R = len(cubes) if R is None else R
    A = min(max(amount, 1), V)
    rp = torch.from_numpy(row_ptr).to(dev)
    ix = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(dev)
    ws = torch.full((int(L.lib().cc_recommend_batch_rank_ws_size(V, d, len(cubes), mn)) // 4 + 64,), -1,
                    device=dev, dtype=torch.int32)
    assert ws.data_ptr() % 256 == 0
    nadd = torch.full((len(cubes),), 77, device=dev, dtype=torch.int32)
    adds = torch.full((len(cubes), A), 77, device=dev, dtype=torch.int32)
    addv = torch.full((len(cubes), A), 7.0, device=dev)
    cutv = torch.full((max(len(idx), 1),), 7.0, device=dev)
    probs = torch.full((len(cubes), V), 7.0, device=dev) if want_probs else None
    rc = L.lib().cc_recommend_batch_rank_fp32(
        L.ptr(rec.params), V, d, R, L.ptr(rp), L.ptr(ix), max_n, amount,
        L.C.c_void_p(ws.data_ptr() + ws_shift), None if null else L.ptr(nadd), L.ptr(adds), L.ptr(addv),
        L.ptr(cutv), L.ptr(probs), L.stream_ptr())
    torch.cuda.synchronize()
    return (rc, row_ptr, idx, nadd.cpu().numpy(), adds.cpu().numpy(), addv.cpu().numpy(), cutv.cpu().numpy(),
            probs.cpu().numpy() if want_probs else None)


@pytest.mark.parametrize('V,d', SHAPES)
def test_direct_call(V, d):
    P, rec = model_of(V, d)
    cubes = mixed_batch(V)
    want = oracle_probs(('mixed', V, d), P, cubes)
    for amount in (2049, V - 1, V, ALL):
        rc, row_ptr, idx, nadd, adds, addv, cutv, probs = _direct(rec, cubes, amount, want_probs=amount == ALL)
        assert rc == 0
        assert adds.shape[1] == min(amount, V)            # the row pitch is clamped to V
        for r, cube in enumerate(cubes):
            exp, _ = infer_ref.top_n(want[r], cube, amount)
            k = len(exp)
            assert nadd[r] == k == min(amount, V - len(np.unique(cube)))
            if amount == ALL:
                assert nadd[r] == V - len(np.unique(cube))
                assert np.array_equal(probs[r], want[r])
            assert np.array_equal(adds[r, :k], exp) and np.array_equal(addv[r, :k], want[r][exp])
            assert np.all(adds[r, k:] == -1) and np.all(addv[r, k:] == 0.0)
            lo, hi = row_ptr[r], row_ptr[r + 1]
            assert np.array_equal(cutv[lo:hi], want[r][idx[lo:hi]])
        assert nadd[7] == 0                                 # n = V: no candidate


@pytest.mark.parametrize('V,d,R', tile_cases.TILE_CASES)
def test_direct_call_tile_shapes(V, d, R):
    """The output tile's edges (tests/tile_cases.py) under the ranking entry."""
    rec, cubes, want = tile_cases.recommender(V, d), tile_cases.cubes(V, R), tile_cases.probs(V, d, R)
    rc, row_ptr, idx, nadd, adds, addv, cutv, probs = _direct(rec, cubes, V, want_probs=True)
    assert rc == 0
    for r, cube in enumerate(cubes):
        exp, _ = infer_ref.top_n(want[r], cube, V)
        k = len(exp)
        assert nadd[r] == k == V - len(cube)
        assert np.array_equal(probs[r], want[r])
        assert np.array_equal(adds[r, :k], exp) and np.array_equal(addv[r, :k], want[r][exp])
        assert np.all(adds[r, k:] == -1) and np.all(addv[r, k:] == 0.0)
        lo, hi = row_ptr[r], row_ptr[r + 1]
        assert np.array_equal(cutv[lo:hi], want[r][idx[lo:hi]])


@pytest.mark.parametrize('V,d', SHAPES)
def test_mixed_batch_bit_exact(V, d):
    P, rec = model_of(V, d)
    cubes = mixed_batch(V)
    want = oracle_probs(('mixed', V, d), P, cubes)
    for amount in (2049, V - 1, V, ALL):
        outs = rec.recommend_many(cubes, amount, want_probs=True)
        assert len(outs) == len(cubes)
        for r, cube in enumerate(cubes):
            check_row(outs[r], want[r], cube, amount, probs=True)
        assert len(outs[7]['additions']) == 0              # n = V: no candidate
        assert len(outs[6]['additions']) == 1              # n = V - 1: one


def test_ties_and_zeros():
    """Long blocks of exact ones and exact zeros: ties that span many waves and all three passes."""
    V, d = 4100, 128
    assert det_sigmoid32(np.float32(40.0)) == np.float32(1.0)
    assert det_sigmoid32(np.float32(-200.0)) == np.float32(0.0)
    P, _ = model_of(V, d)
    P2 = dict(P)
    i = np.arange(V)
    P2['decoder/reconstruct/bias'] = np.where(i % 3 == 0, 40.0, np.where(i % 3 == 1, -200.0, -3.0)).astype(np.float32)
    rec = Recommender(Layout(V, d).pack(P2), V, d)
    cubes = [np.arange(0, 300, 7), np.zeros(0, np.int64), np.arange(V - 60, V), np.arange(0, V, 3)[5:200]]
    want = oracle_probs(('ties', V, d), P2, cubes)
    assert all(np.sum(w == 1.0) > 1000 and np.sum(w == 0.0) > 1000 for w in want)
    outs = rec.recommend_many(cubes, ALL)
    for r, cube in enumerate(cubes):
        check_row(outs[r], want[r], cube, ALL)             # the full ranking
        adds, vals = outs[r]['additions'], outs[r]['add_vals']
        in_cube = np.zeros(V, bool)
        in_cube[cube] = True
        assert len(adds) == V - in_cube.sum() and not in_cube[adds].any()
        for tie in (1.0, 0.0):
            assert np.all(np.diff(adds[vals == tie]) < 0)  # equal values: higher card index first
        zeros = np.flatnonzero((want[r] == 0.0) & ~in_cube)
        assert np.array_equal(adds[len(adds) - len(zeros):], zeros[::-1])   # all there, at the very end
        assert np.all(vals[:len(adds) - len(zeros)] > 0.0)


def test_routing_stays_off_the_single_cube_path():
    V, d = 1001, 128
    P, _ = model_of(V, d)
    rec = Recommender(Layout(V, d).pack(P), V, d)
    cubes = mixed_batch(V)
    want = oracle_probs(('mixed', V, d), P, cubes)

    def refuse(*a, **k):
        raise AssertionError('recommend_many fell back to recommend')
    rec.recommend = refuse
    outs = rec.recommend_many(cubes, limit() + 1)
    for r, cube in enumerate(cubes):
        check_row(outs[r], want[r], cube, limit() + 1)


def test_agrees_with_the_single_cube_path():
    V, d = 1001, 128
    _, rec = model_of(V, d)
    cubes = mixed_batch(V)
    many = rec.recommend_many(cubes, ALL, want_probs=True)
    for r, cube in enumerate(cubes):
        one = rec.recommend(cube, ALL, want_probs=True)
        assert sorted(one) == sorted(many[r])
        for key in one:
            assert one[key].dtype == many[r][key].dtype
            assert np.array_equal(one[key], many[r][key]), (r, key)


def test_chunks_and_row_independence():
    V, d = 1001, 128
    P, rec = model_of(V, d)
    cubes = random_cubes(V, 130, seed=5)
    want = oracle_probs(('random130', V, d), P, cubes)
    a = rec.recommend_many(cubes, ALL, want_probs=True, rows_per_launch=512)
    b = rec.recommend_many(cubes, ALL, want_probs=True, rows_per_launch=32)   # uneven: 4 x 32 + 2
    assert len(a) == len(b) == 130
    for r in range(130):
        check_row(a[r], want[r], cubes[r], ALL, probs=True)
        for key in ('additions', 'add_vals', 'cut_vals', 'probs'):
            assert np.array_equal(a[r][key], b[r][key]), (r, key)
    alone = rec.recommend_many([cubes[77]], ALL, want_probs=True)[0]
    for key in alone:
        assert np.array_equal(alone[key], a[77][key]), key


def test_workspace_state_does_not_leak():
    """The larger batch first: its keys, bitmasks and sorted pairs sit beyond the second batch's."""
    V, d = 1001, 128
    P, _ = model_of(V, d)
    rec = Recommender(Layout(V, d).pack(P), V, d)
    big, small = random_cubes(V, 130, seed=5), mixed_batch(V)
    want_big = oracle_probs(('random130', V, d), P, big)
    want_small = oracle_probs(('mixed', V, d), P, small)
    for cubes, want in ((big, want_big), (small, want_small)):
        outs = rec.recommend_many(cubes, ALL)
        for r, cube in enumerate(cubes):
            check_row(outs[r], want[r], cube, ALL)


def test_guards():
    V, d = 63, 64
    _, rec = model_of(V, d)
    cubes = [[1, 2, 3], [4]]
    assert _direct(rec, cubes, ALL)[0] == 0
    assert _direct(rec, cubes, ALL, null=True)[0] == -1    # CC_ERR_ARG
    assert b'null' in L.lib().cc_last_error_string()
    assert _direct(rec, cubes, ALL, ws_shift=4)[0] == -1
    assert b'aligned' in L.lib().cc_last_error_string()
    assert _direct(rec, cubes, ALL, max_n=V + 1)[0] == -1
    rc, _, _, nadd, adds, _, _, _ = _direct(rec, cubes, ALL, R=0)
    assert rc == 0 and np.all(nadd == 77) and np.all(adds == 77)   # CC_OK, nothing launched
    with pytest.raises(ValueError):
        rec.recommend_many([[1, 2], [3, V]], ALL)
    with pytest.raises(ValueError):
        rec.recommend_many([[-1]], ALL)
    assert rec.recommend_many([], ALL) == []


def test_full_shape():
    V, d = 20884, 512                                      # the reference checkpoint's architecture
    P = model_ref.init_params(V, d, seed=20250301, bias_std=0.01)
    rec = Recommender(Layout(V, d).pack(P), V, d)
    rng = np.random.default_rng(64)
    cubes = [rng.choice(V, int(rng.integers(45, 721)), replace=False) for _ in range(8)]
    outs = rec.recommend_many(cubes, ALL)
    assert len(outs) == 8
    for r in (0, 7):
        assert len(outs[r]['additions']) == V - len(cubes[r])
        check_row(outs[r], infer_ref.recommend_probs(P, cubes[r]), cubes[r], ALL)


def test_web_function_matches_get_ml_recommend(tmp_path):
    from cubecobrarecommender_amd import checkpoint as ck
    V, d = 300, 64
    P = model_ref.init_params(V, d, seed=3, bias_std=0.01)
    dest = str(tmp_path / 'ml_files' / 'recommender')
    ck.save_model(dest, V, d, P)
    names = {i: f'card {i}' for i in range(V)}
    idmap = tmp_path / 'id_map.json'
    idmap.write_text(json.dumps({str(k): v for k, v in names.items()}))
    root = tmp_path / 'site'
    (root / 'cube' / 'api' / 'cubelist').mkdir(parents=True)
    rng = np.random.default_rng(9)
    cube_names = ['first', 'second', 'empty']
    for name, n in zip(cube_names, (40, 7, 0)):
        cards = [names[int(c)] for c in rng.choice(V, n, replace=False)]
        (root / 'cube' / 'api' / 'cubelist' / name).write_text('\n'.join(cards + ['custom card']))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from web.ml_recommend_web import get_ml_recommend, get_ml_recommend_many
    kw = dict(root=str(root), model_dir=dest, id_map=str(idmap))
    many = get_ml_recommend_many(cube_names, ALL, **kw)
    assert len(many) == 3
    for name, got in zip(cube_names, many):
        one = get_ml_recommend(name, ALL, **kw)
        assert got == one and list(got['additions']) == list(one['additions'])
        assert list(got['cuts']) == list(one['cuts'])
    assert len(many[0]['additions']) == V - 40 and len(many[2]['additions']) == V
