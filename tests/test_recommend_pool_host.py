"""CPU tests of the card pools' host side: pool_words / CardPool, the argument errors that must come
before any launch, the six cc_recommend_batch_*pool* bindings against include/ccrec.h, api.load_pool
and evaluate_holdout(pool=)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api
from cubecobrarecommender_amd.evaluate import evaluate_holdout, holdout_split, metrics_from_ranks
from cubecobrarecommender_amd.recommender import CardPool, Recommender, pool_words, resolve_pools

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ccrec.h')
VS = [1, 31, 32, 33, 63, 64, 1001]


def bits_of(words, n):
    """words -> bool [n]: bit j & 31 of word j >> 5."""
    j = np.arange(n)
    return ((words[j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


@pytest.mark.parametrize('V', VS)
def test_pool_words(V):
    VW = (V + 31) // 32
    rng = np.random.default_rng(V)
    some = rng.choice(V, max(1, V // 3), replace=False)
    cases = [[], [V - 1], [0], np.arange(V), some, np.concatenate([some[::-1], some[:5], some[:1]])]
    for ids in cases:
        w = pool_words(ids, V)
        assert w.dtype == np.uint32 and w.shape == (VW,)
        want = np.zeros(32 * VW, bool)
        want[np.asarray(ids, np.int64)] = True
        assert np.array_equal(bits_of(w, 32 * VW), want)        # the ids' bits, and none at or above V
        assert not bits_of(w, 32 * VW)[V:].any()
    assert not pool_words([], V).any()
    w = pool_words([V - 1], V)
    assert w[VW - 1] == np.uint32(1) << ((V - 1) & 31) and not w[:VW - 1].any()
    assert np.array_equal(pool_words(some, V), pool_words(np.sort(some), V))   # order does not matter
    for bad in (-1, V):
        with pytest.raises(ValueError, match='outside'):
            pool_words([0, bad], V)
        with pytest.raises(ValueError, match='outside'):
            CardPool([bad], V)


def test_card_pool():
    p = CardPool([9, 3, 3, 40, 9], 41)
    assert p.ids.tolist() == [3, 9, 40] and p.size == 3 and p.V == 41
    assert np.array_equal(p.words, pool_words([3, 9, 40], 41)) and p.words_dev is None
    assert p.contains([3, 4, 40, 0, 41, -1, 10 ** 9]).tolist() == [True, False, True, False, False, False, False]
    empty = CardPool([], 41)
    assert empty.size == 0 and not empty.words.any() and not empty.contains([0, 40]).any()


def test_resolve_pools():
    a, b = CardPool([1, 2], 50), CardPool([2, 3], 50)
    assert resolve_pools(None, 3, 50) == (None, None)
    assert resolve_pools([None, None], 2, 50) == (None, None)       # nothing pooled: the unpooled call
    pools, por = resolve_pools(a, 3, 50)
    assert pools == [a] and por.dtype == np.int32 and por.tolist() == [0, 0, 0]
    pools, por = resolve_pools([b, None, a, b, a], 5, 50)           # distinct pools once, first use first
    assert pools == [b, a] and por.tolist() == [0, -1, 1, 0, 1]
    assert resolve_pools(a, 0, 50)[0] is None


def bare_recommender(V=50, d=64):
    rec = Recommender.__new__(Recommender)                          # no device, no weights: nothing can launch
    rec.V, rec.d, rec.dev = V, d, None
    return rec


def test_argument_errors_come_before_any_launch():
    rec = bare_recommender()
    good, other = CardPool([5, 6, 7, 8], 50), CardPool([5, 6], 49)
    cubes = [[1, 2, 3], [4]]
    for call in (lambda **kw: rec.recommend_many(cubes, 10, **kw),
                 lambda **kw: rec.recommend_many(cubes, 30000, **kw),
                 lambda **kw: rec.target_ranks(cubes, [[5], [6]], **kw)):
        with pytest.raises(ValueError, match='built for 49 cards'):
            call(pool=other)
        with pytest.raises(ValueError, match=r'cube 1.*built for 49'):
            call(pool=[good, other])
        with pytest.raises(ValueError, match='3 pools for 2 cubes'):
            call(pool=[good, None, good])
        with pytest.raises(ValueError, match='1 pools for 2 cubes'):
            call(pool=[good])
        with pytest.raises(ValueError, match='not a CardPool'):
            call(pool=[good, [5, 6]])
    with pytest.raises(ValueError, match='built for 49'):
        rec.recommend(cubes[0], 10, pool=other)
    with pytest.raises(ValueError, match='want_order'):
        rec.recommend(cubes[0], 10, want_order=True, pool=good)
    # a target outside its row's pool: the cube and the card are named
    with pytest.raises(ValueError, match='cube 1: target card 9 is outside the pool'):
        rec.target_ranks(cubes, [[5, 8], [6, 9]], pool=good)
    with pytest.raises(ValueError, match='cube 0: target card 30 is outside the pool'):
        rec.target_ranks(cubes, [[30], [6, 9]], pool=[good, None])
    # the earlier rules still come first / still hold with a pool
    with pytest.raises(ValueError, match='cube 1: target card 4 is in the cube'):
        rec.target_ranks(cubes, [[5], [4]], pool=CardPool([4, 5], 50))
    with pytest.raises(ValueError, match='outside'):
        rec.recommend_many([[1, 50]], 10, pool=CardPool([1], 50))
    assert rec.recommend_many([], 10, pool=good) == []
    assert rec.target_ranks([], [], pool=good) == ([], [], None)


# ---------------------------------------------------------------------------------- bindings
POOLED = {'cc_recommend_batch_pool': 'cc_recommend_batch',
          'cc_recommend_batch_rank_pool': 'cc_recommend_batch_rank',
          'cc_recommend_batch_target_ranks_pool': 'cc_recommend_batch_target_ranks'}


def header_args(name):
    """The parameter declarations of `name` in include/ccrec.h."""
    text = open(HEADER).read()
    m = re.search(r'^(?:int|size_t) ' + name + r'\s*\(([^;]*?)\)\s*;', text, re.S | re.M)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_bindings():
    p, i32 = C.c_void_p, C.c_int32
    for pooled, plain in POOLED.items():
        assert L.SIGNATURES[pooled + '_ws_size'] == (C.c_size_t, [i32, i32, i32, i32])
        res, args = L.SIGNATURES[plain + '_fp32']
        # the unpooled entry's arguments, then pools, n_pools, pool_of_row, then the stream
        assert L.SIGNATURES[pooled + '_fp32'] == (res, args[:-1] + [p, i32, p] + args[-1:])
        for suffix in ('_ws_size', '_fp32'):
            assert len(header_args(pooled + suffix)) == len(L.SIGNATURES[pooled + suffix][1])
        decl = header_args(pooled + '_fp32')
        assert decl[:-4] == header_args(plain + '_fp32')[:-1]
        assert [re.sub(r'\s+', ' ', a) for a in decl[-4:]] == [
            'const uint32_t *pools', 'int32_t n_pools', 'const int32_t *pool_of_row', 'void *stream']
    assert len(L.SIGNATURES['cc_recommend_batch_pool_fp32'][1]) == 18
    assert len(L.SIGNATURES['cc_recommend_batch_rank_pool_fp32'][1]) == 18
    assert len(L.SIGNATURES['cc_recommend_batch_target_ranks_pool_fp32'][1]) == 21
    lib = L.lib()
    assert lib.cc_abi_version() == 2
    for pooled in POOLED:
        assert getattr(lib, pooled + '_ws_size').restype is C.c_size_t
        assert getattr(lib, pooled + '_fp32').restype is C.c_int


def test_workspace_sizes():
    lib = L.lib()
    for V, d, R, max_n in [(1, 64, 1, 0), (63, 64, 11, 63), (1001, 128, 70, 500), (20884, 512, 512, 720)]:
        VW = (V + 31) // 32
        for pooled, plain in POOLED.items():
            a = int(getattr(lib, pooled + '_ws_size')(V, d, R, max_n))
            b = int(getattr(lib, plain + '_ws_size')(V, d, R, max_n))
            assert a % 256 == 0 and a >= b + 4 * R * VW + 4 * R      # the exclusion rows and the counts
            assert a <= b + 4 * R * VW + 4 * R + 512                 # and nothing else (two 256-B roundings)


# ---------------------------------------------------------------------------------- load_pool
def test_load_pool(tmp_path):
    card_to_int = {'lim-dul the necromancer': 0, 'juzam djinn': 1, 'aether vial': 2, 'seance': 3, 'bog': 4}
    f = tmp_path / 'pool.txt'
    f.write_text('Lim-Dûl the Necromancer\nJUZÁM DJINN\n\nMy Custom Card\nÆther Vial\n  Séance  \nbog\nbog\n'
                 'another unknown\n', encoding='utf8')
    ids, n_unknown = api.load_pool(str(f), card_to_int)
    assert ids == [0, 1, 2, 3, 4, 4] and n_unknown == 2             # the empty line is no name
    assert CardPool(ids, 5).size == 5
    f.write_text('', encoding='utf8')
    assert api.load_pool(str(f), card_to_int) == ([], 0)


# ---------------------------------------------------------------------------------- evaluate_holdout
class StubRecommender:
    """target_ranks records its arguments and ranks target t of a cube at t % 7."""

    def __init__(self):
        self.calls = []

    def target_ranks(self, cubes, targets, cutoffs=(), rows_per_launch=512, pool=None):
        self.calls.append(dict(cubes=cubes, targets=targets, cutoffs=cutoffs, rows_per_launch=rows_per_launch,
                               pool=pool))
        ranks = [np.asarray(t, np.int64) % 7 for t in targets]
        return ranks, [np.zeros(len(t), np.float32) for t in targets], None


class OldStub:
    def __init__(self):
        self.calls = []

    def target_ranks(self, cubes, targets, cutoffs=(), rows_per_launch=512):
        self.calls.append((cubes, targets))
        return [np.asarray(t, np.int64) % 7 for t in targets], None, None


def test_evaluate_holdout_pool():
    V = 60
    rng = np.random.default_rng(2)
    cubes = [rng.choice(V, n, replace=False) for n in (20, 1, 35, 12, 0, 50)]
    visible, hidden = holdout_split(cubes, hide=0.4, seed=3)
    evens, low = CardPool(np.arange(0, V, 2), V), CardPool(np.arange(0, 25), V)

    stub = StubRecommender()
    got = evaluate_holdout(stub, cubes, ks=(2, 5), hide=0.4, seed=3)          # pool=None: as before
    call = stub.calls[0]
    assert call['pool'] is None and 'n_targets_outside_pool' not in got
    assert all(np.array_equal(a, b) for a, b in zip(call['targets'], hidden)) and len(call['targets']) == len(hidden)
    assert all(np.array_equal(a, b) for a, b in zip(call['cubes'], visible))
    old = OldStub()                                                             # a model without pools still works
    assert evaluate_holdout(old, cubes, ks=(2, 5), hide=0.4, seed=3) == got
    assert all(np.array_equal(a, b) for a, b in zip(old.calls[0][1], hidden))

    for pool, per_row in ((evens, [evens] * 6), ([evens, None, low, low, None, evens],) * 2):
        stub = StubRecommender()
        got = evaluate_holdout(stub, cubes, ks=(2, 5), hide=0.4, seed=3, rows_per_launch=9, pool=pool)
        call = stub.calls[0]
        kept = [h if p is None else h[p.contains(h)] for h, p in zip(hidden, per_row)]
        assert call['pool'] is pool and call['rows_per_launch'] == 9 and tuple(call['cutoffs']) == (2, 5)
        assert all(np.array_equal(a, b) for a, b in zip(call['cubes'], visible))     # the unpooled split
        assert all(np.array_equal(a, b) for a, b in zip(call['targets'], kept))
        dropped = sum(len(h) for h in hidden) - sum(len(k) for k in kept)
        assert dropped > 0 and got.pop('n_targets_outside_pool') == dropped
        assert got == metrics_from_ranks([k % 7 for k in kept], (2, 5))             # over the remaining cards
        assert got['n_targets'] == sum(len(k) for k in kept)

    with pytest.raises(ValueError, match='takes no pool'):
        evaluate_holdout(OldStub(), cubes, pool=evens)
    with pytest.raises(ValueError, match='5 pools for 6 cubes'):
        evaluate_holdout(StubRecommender(), cubes, pool=[evens] * 5)


def test_graph_recommender_has_no_pools():
    from cubecobrarecommender_amd import graphrec
    rec = graphrec.GraphRecommender.__new__(graphrec.GraphRecommender)         # no device, no graph
    rec.V = 50
    with pytest.raises(ValueError, match='takes no pool'):
        evaluate_holdout(rec, [[1, 2, 3]], pool=CardPool([1, 2], 50))
