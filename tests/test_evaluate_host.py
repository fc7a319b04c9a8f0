"""CPU tests of the held-out evaluation's host side: holdout_split, pack_targets,
metrics_from_ranks against hand-worked cases, and the two cc_recommend_batch_target_ranks_*
bindings."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.evaluate import holdout_split, metrics_from_ranks
from cubecobrarecommender_amd.recommender import pack_cubes, pack_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def some_cubes():
    rng = np.random.default_rng(11)
    cubes = [rng.choice(500, int(n), replace=False) for n in (0, 1, 2, 3, 5, 10, 37, 100, 360)]
    cubes.append(np.array([7, 7, 9, 9, 9, 3, 3, 1, 250, 250]))          # duplicates: 5 distinct
    return cubes


def test_holdout_split_is_a_partition_and_reproducible():
    cubes = some_cubes()
    vis, hid = holdout_split(cubes, hide=0.2, seed=4)
    vis2, hid2 = holdout_split(cubes, hide=0.2, seed=4)
    assert len(vis) == len(hid) == len(cubes)
    for c, v, h, v2, h2 in zip(cubes, vis, hid, vis2, hid2):
        assert np.array_equal(v, v2) and np.array_equal(h, h2)
        u = np.unique(c)
        assert len(np.intersect1d(v, h)) == 0
        assert np.array_equal(np.sort(np.concatenate([v, h])), u)       # the distinct cube, once each
        n = len(u)
        want = 0 if n < 2 else max(1, int(math.floor(0.2 * n)))
        assert len(h) == want, n
    assert [len(h) for h in hid] == [0, 0, 1, 1, 1, 2, 7, 20, 72, 1]
    _, hid3 = holdout_split(cubes, hide=0.2, seed=5)
    assert any(not np.array_equal(a, b) for a, b in zip(hid, hid3))    # the seed matters


def test_holdout_split_count_form_and_min_visible():
    cubes = some_cubes()
    vis, hid = holdout_split(cubes, hide=3, seed=0)
    # a count, capped so that one card stays visible
    assert [len(h) for h in hid] == [0, 0, 1, 2, 3, 3, 3, 3, 3, 3]
    assert all(len(v) >= 1 or len(np.unique(c)) == 0 for c, v in zip(cubes, vis))
    vis, hid = holdout_split(cubes, hide=0.5, min_visible=4, seed=0)
    assert [len(h) for h in hid] == [0, 0, 0, 0, 1, 5, 18, 50, 180, 1]
    assert [len(v) for v in vis] == [0, 1, 2, 3, 4, 5, 19, 50, 180, 4]
    vis, hid = holdout_split(cubes, hide=0, seed=0)
    assert all(len(h) == 0 for h in hid)
    with pytest.raises(ValueError):
        holdout_split(cubes, hide=2.5)
    with pytest.raises(ValueError):
        holdout_split(cubes, hide=-0.1)
    assert holdout_split([]) == ([], [])


def test_pack_targets_round_trip():
    V = 50
    cubes = [[5, 3, 3, 9], [], [0, 49], [1]]
    targets = [[10, 2, 10, 48, 4], [7], [], [49, 0, 0]]                 # unsorted, duplicates, empty
    _, _, _, inputs, _ = pack_cubes(cubes, V)
    tgt_ptr, tgt = pack_targets(targets, inputs, V)
    assert tgt_ptr.dtype == np.int32 and tgt.dtype == np.int32
    assert tgt_ptr.tolist() == [0, 5, 6, 6, 9]
    for r, t in enumerate(targets):
        assert tgt[tgt_ptr[r]:tgt_ptr[r + 1]].tolist() == t             # the caller's order, duplicates kept
    tp, tg = pack_targets([], [], V)
    assert tp.tolist() == [0] and len(tg) == 0


def test_pack_targets_errors():
    V = 50
    _, _, _, inputs, _ = pack_cubes([[5, 3], [7, 8]], V)
    with pytest.raises(ValueError, match=r'cube 1.*outside'):
        pack_targets([[1], [2, V]], inputs, V)
    with pytest.raises(ValueError, match='outside'):
        pack_targets([[-1], []], inputs, V)
    with pytest.raises(ValueError, match=r'cube 1: target card 8 is in the cube'):
        pack_targets([[7], [2, 8]], inputs, V)                          # 7 is in cube 1, not in cube 0
    with pytest.raises(ValueError):
        pack_targets([[1]], inputs, V)                                  # one list per cube


def test_metrics_all_hits():
    m = metrics_from_ranks([np.array([0, 1, 2])], ks=(3, 10))
    for K in (3, 10):
        assert m[f'recall@{K}'] == 1.0 and m[f'hit_rate@{K}'] == 1.0
        assert m[f'ndcg@{K}'] == pytest.approx(1.0, abs=1e-15)          # the ideal order itself
    assert m['mrr'] == 1.0 and m['n_cubes'] == 1 and m['n_targets'] == 3


def test_metrics_straddling_k_by_hand():
    ranks = [np.array([0, 4, 5, 40], np.int32),      # K = 5: ranks 0 and 4 hit, 5 just misses
             np.zeros(0, np.int32),                  # no hidden card: in no per-cube mean
             np.array([9, 2], np.int32),             # unsorted
             np.array([7], np.int32)]
    m = metrics_from_ranks(ranks, ks=(5, 1))
    assert m['n_cubes'] == 3 and m['n_targets'] == 7
    assert m['recall@5'] == 3 / 7 and m['recall@1'] == 1 / 7
    l2 = math.log2
    idcg4 = 1 / l2(2) + 1 / l2(3) + 1 / l2(4) + 1 / l2(5)              # min(5, 4 hidden)
    idcg2 = 1 / l2(2) + 1 / l2(3)
    ndcg5 = ((1 / l2(2) + 1 / l2(6)) / idcg4 + (1 / l2(4)) / idcg2 + 0.0) / 3
    assert m['ndcg@5'] == pytest.approx(ndcg5, rel=1e-14)
    assert m['ndcg@1'] == pytest.approx((1.0 + 0.0 + 0.0) / 3, rel=1e-14)   # ideal DCG at K = 1 is 1
    assert m['hit_rate@5'] == pytest.approx(2 / 3) and m['hit_rate@1'] == pytest.approx(1 / 3)
    assert m['mrr'] == pytest.approx((1 / 1 + 1 / 3 + 1 / 8) / 3, rel=1e-14)
    assert all(isinstance(m[k], float) for k in m if k not in ('n_cubes', 'n_targets'))


def test_metrics_ignore_invalid_ranks_and_empty_input():
    a = metrics_from_ranks([np.array([-1, 3, -1]), np.array([-1])], ks=(4,))
    b = metrics_from_ranks([np.array([3])], ks=(4,))
    assert a == b and a['n_cubes'] == 1 and a['n_targets'] == 1
    e = metrics_from_ranks([], ks=(10,))
    assert e == {'recall@10': 0.0, 'ndcg@10': 0.0, 'hit_rate@10': 0.0, 'mrr': 0.0, 'n_cubes': 0, 'n_targets': 0}


def header_arg_count(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])


def test_lib_declares_the_two_symbols_with_the_headers_argument_counts():
    i32, P = C.c_int32, C.c_void_p
    size, entry = 'cc_recommend_batch_target_ranks_ws_size', 'cc_recommend_batch_target_ranks_fp32'
    assert L.SIGNATURES[size] == (C.c_size_t, [i32, i32, i32, i32])
    assert L.SIGNATURES[entry] == (C.c_int, [P, i32, i32, i32, P, P, i32, P, P, P, i32, P, P, P, P, P, P, P])
    assert len(L.SIGNATURES[size][1]) == header_arg_count(size) == 4
    assert len(L.SIGNATURES[entry][1]) == header_arg_count(entry) == 18
    lib = L.lib()
    assert lib.cc_recommend_batch_target_ranks_ws_size.restype is C.c_size_t
    # the batch workspace and nothing more: no ping-pong buffers
    for V, d, R, max_n in ((63, 64, 1, 0), (1001, 128, 11, 500), (20884, 512, 512, 540)):
        assert int(lib.cc_recommend_batch_target_ranks_ws_size(V, d, R, max_n)) == int(
            lib.cc_recommend_batch_ws_size(V, d, R, max_n))
        assert int(lib.cc_recommend_batch_target_ranks_ws_size(V, d, R, max_n)) < int(
            lib.cc_recommend_batch_rank_ws_size(V, d, R, max_n))


def test_argument_errors_need_no_gpu():
    """The checks come before any launch: null pointer, n_cutoffs, workspace alignment, R == 0."""
    lib = L.lib()
    one = C.c_void_p(4096)                           # never dereferenced: every call fails or has R == 0
    f = lib.cc_recommend_batch_target_ranks_fp32

    def call(R=2, ranks=one, n_cut=0, cutoffs=None, ws=one, V=63, max_n=3):
        return f(one, V, 64, R, one, one, max_n, one, one, cutoffs, n_cut, ws, ranks, one, None, one, None, None)
    assert call(ranks=None) == -1 and b'null' in lib.cc_last_error_string()
    assert call(n_cut=9, cutoffs=one) == -1 and b'n_cutoffs' in lib.cc_last_error_string()
    assert call(n_cut=-1) == -1
    assert call(n_cut=2, cutoffs=None) == -1
    assert call(ws=C.c_void_p(4096 + 4)) == -1 and b'aligned' in lib.cc_last_error_string()
    assert call(max_n=64) == -1 and b'max_n' in lib.cc_last_error_string()
    assert call(R=0) == 0                            # CC_OK, nothing launched
