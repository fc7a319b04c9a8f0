"""CPU tests of the diverse re-ranking's host side: the reference loop's own properties
(tests/diverse_ref.py) and a hand-worked case, the three bindings against the header, the argument
checks of cc_recommend_diverse_fp32 with never-dereferenced pointers, the workspace size, the
planning functions and every ValueError that comes before a launch, the api wrapper and the CLI."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api, diverse
from cubecobrarecommender_amd.recommender import CardPool
from tests import diverse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------ the reference loop
def descending_p(rng, n):
    return np.sort(rng.random(n).astype(f32))[::-1].copy()


def test_trade_one_is_the_identity():
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((50, 16)).astype(f32)
    c, p = rng.permutation(50)[:30], descending_p(rng, 30)
    for amount in (0, 1, 7, 30, 35):
        ids, vals, red, rank = diverse_ref.mmr(c, p, emb, amount, 1.0)
        k = min(max(amount, 1), 30)
        assert rank.tolist() == list(range(k)) and np.array_equal(ids, c[:k]) and np.array_equal(u32(vals), u32(p[:k]))
        assert ids.dtype == np.int32 and rank.dtype == np.int32 and vals.dtype == red.dtype == f32
    for got in diverse_ref.mmr([], [], emb, 5, 0.5):
        assert len(got) == 0


def test_zero_embeddings_give_the_base_order():
    rng = np.random.default_rng(2)
    c, p = rng.permutation(40)[:25], descending_p(rng, 25)
    p[3] = p[4] = p[5]                                              # ties in p keep the base order too
    for trade in (0.0, 0.3, 0.7, 1.0):
        ids, vals, red, rank = diverse_ref.mmr(c, p, np.zeros((40, 8), f32), 25, trade)
        assert rank.tolist() == list(range(25)) and np.all(u32(red) == 0)


def test_twins_wait_while_an_untouched_pair_exists():
    """Every embedding twice, equal p: a card's twin has the greatest redundancy there is, so the
    first half of the picks takes one card of every pair."""
    rng = np.random.default_rng(3)
    pairs = 12
    emb = np.repeat(rng.standard_normal((pairs, 64)).astype(f32), 2, axis=0)
    c = rng.permutation(2 * pairs)
    p = np.full(2 * pairs, 0.5, f32)
    for trade in (0.0, 0.3, 0.7):
        ids, _, red, rank = diverse_ref.mmr(c, p, emb, 2 * pairs, trade)
        assert sorted(ids.tolist()) == list(range(2 * pairs))
        assert sorted((ids[:pairs] // 2).tolist()) == list(range(pairs))
        assert np.all(red[:pairs] < 0.9) and np.all(red[pairs:] > 0.999)
        assert rank[0] == 0


def test_hand_worked_case():
    """Five candidates, one-hot rows (sims exactly 0 or 1), trade 0.5: every number below is exact.
         j      0      1      2      3      4
         p      .875   .75    .625   .5     .375
         row    e0     e0     e1     e0     e2
      t0 scores .4375  .375   .3125  .25    .1875 -> 0; red = [-, 1, 0, 1, 0]
      t1 scores        -.125  .3125  -.25   .1875 -> 2; nothing is like e1
      t2 scores        -.125         -.25   .1875 -> 4
      t3 -> 1, t4 -> 3, both charged 1."""
    emb = np.zeros((9, 4), f32)
    cards = [8, 2, 5, 0, 3]
    for card, hot in zip(cards, (0, 0, 1, 0, 2)):
        emb[card, hot] = 3.0
    p = np.array([.875, .75, .625, .5, .375], f32)
    ids, vals, red, rank = diverse_ref.mmr(cards, p, emb, 5, 0.5)
    assert rank.tolist() == [0, 2, 4, 1, 3] and ids.tolist() == [8, 5, 3, 2, 0]
    assert vals.tolist() == [.875, .625, .375, .75, .5] and red.tolist() == [0, 0, 0, 1, 1]
    ids, _, red, rank = diverse_ref.mmr(cards, p, emb, 3, 0.5)
    assert rank.tolist() == [0, 2, 4]
    # trade .875 charges a twin .125: t1 .53125 < .546875 -> 2, t2 -> 1, t3 .3125 < .328125 -> 4, t4 -> 3
    ids, _, red, rank = diverse_ref.mmr(cards, p, emb, 5, 0.875)
    assert rank.tolist() == [0, 2, 1, 4, 3] and red.tolist() == [0, 0, 1, 0, 1]


def test_a_negative_similarity_never_replaces_the_zero():
    emb = np.array([[1, 0], [-1e-30, 1], [0, 1]], f32)             # sim(0, 1) is just below zero
    _, _, red, rank = diverse_ref.mmr([0, 1, 2], [.5, .5, .5], emb, 3, 0.5)
    assert rank.tolist() == [0, 1, 2] and u32(red)[1] == 0


# ------------------------------------------------------------------------------ the C entry
def header_args(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return [a.strip() for a in args.split(',') if a.strip() and a.strip() != 'void']


def test_signatures_match_the_header():
    i32, P, SZ, F = C.c_int32, C.c_void_p, C.c_size_t, C.c_float
    assert L.SIGNATURES['cc_recommend_diverse_max_candidates'] == (i32, [])
    assert L.SIGNATURES['cc_recommend_diverse_ws_size'] == (SZ, [i32] * 6)
    assert L.SIGNATURES['cc_recommend_diverse_fp32'] == (
        C.c_int, [P, i32, i32, i32, P, P, i32, i32, i32, F, P, i32, P, i32, P, i32, P, P, P, P, P, P, P, SZ, P])
    lib = L.lib()
    for name, count in (('cc_recommend_diverse_max_candidates', 0), ('cc_recommend_diverse_ws_size', 6),
                        ('cc_recommend_diverse_fp32', 25)):
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert lib.cc_abi_version() == 2
    assert 256 <= lib.cc_recommend_diverse_max_candidates() <= lib.cc_recommend_batch_max_amount()


def test_workspace_size():
    lib = L.lib()
    ws = lambda R, n, M, K=64, V=22000, d=256: int(lib.cc_recommend_diverse_ws_size(V, d, R, n, M, K))   # noqa: E731
    base = ws(64, 360, 256)
    assert base % 256 == 0
    chain = int(lib.cc_recommend_batch_pool_ws_size(22000, 256, 64, 360)) - 256
    own = 64 * 4 + 2 * 64 * 256 * 4                                 # counts, candidates, probabilities
    assert chain + own <= base <= chain + own + 4 * 256            # R x M words: nothing of size R x V of its own
    assert ws(64, 360, 256) < ws(64, 360, 512) and ws(64, 360, 256) < ws(65, 360, 256)
    assert ws(64, 360, 256, K=40) == ws(64, 360, 256, K=96)         # the embeddings live in LDS
    assert ws(0, 0, 0) > 0


def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    top = lib.cc_recommend_diverse_max_candidates()
    need = int(lib.cc_recommend_diverse_ws_size(100, 64, 2, 40, top, 64))

    def call(params=one, V=100, d=64, R=2, row_ptr=one, idx=one, max_n=40, amount=10, M=64, lam=0.5, emb=one, K=64,
             pools=None, n_pools=0, pool_of_row=None, A=10, n_add=one, additions=one, add_vals=one, redundancy=one,
             base_rank=one, cut_vals=one, ws=one, ws_bytes=need):
        return lib.cc_recommend_diverse_fp32(params, V, d, R, row_ptr, idx, max_n, amount, M, lam, emb, K, pools,
                                             n_pools, pool_of_row, A, n_add, additions, add_vals, redundancy,
                                             base_rank, cut_vals, ws, ws_bytes, None)

    def failed(what):
        msg = lib.cc_last_error_string()
        return b'cc_recommend_diverse_fp32' in msg and what in msg
    bad = [(dict(params=None), b'null'), (dict(row_ptr=None), b'null'), (dict(idx=None), b'null'),
           (dict(emb=None), b'null'), (dict(n_add=None), b'null'), (dict(additions=None), b'null'),
           (dict(add_vals=None), b'null'), (dict(redundancy=None), b'null'), (dict(base_rank=None), b'null'),
           (dict(cut_vals=None), b'null'), (dict(ws=None), b'null'),
           (dict(pools=one, n_pools=1), b'null'), (dict(n_pools=1), b'null'),
           (dict(pool_of_row=one, n_pools=-1), b'n_pools'), (dict(pool_of_row=one, n_pools=2), b'pools is null'),
           (dict(d=0), b'd must be'), (dict(d=96), b'd must be'), (dict(max_n=101), b'max_n'), (dict(V=0), b'V'),
           (dict(R=-1), b'R'), (dict(K=0), b'K'),
           (dict(lam=-0.001), b'lambda'), (dict(lam=1.001), b'lambda'), (dict(lam=float('nan')), b'lambda'),
           (dict(M=0), b'M outside'), (dict(M=top + 1, ws_bytes=1 << 40), b'M outside'),
           (dict(M=top, K=65), b'LDS'), (dict(M=342, K=96), b'LDS'), (dict(M=128, K=300), b'LDS'),
           (dict(A=9), b'A below'), (dict(amount=100, M=64, A=63), b'A below'), (dict(amount=0, A=0), b'A below'),
           (dict(ws=C.c_void_p(4096 + 64)), b'aligned'), (dict(ws_bytes=0), b'workspace'),
           (dict(M=top, A=10, ws_bytes=need - 1), b'workspace')]
    for kw, what in bad:
        assert call(**kw) == -1 and failed(what), kw
    # R == 0: CC_OK, nothing launched; the limits themselves are legal
    assert call(R=0) == 0 and call(R=0, lam=0.0) == 0 and call(R=0, lam=1.0) == 0
    assert call(R=0, M=top, K=64) == 0 and call(R=0, M=341, K=96) == 0 and call(R=0, M=1, A=1) == 0
    assert call(R=0, amount=100, M=64, A=64) == 0 and call(R=0, amount=0, A=1) == 0
    assert call(R=0, pool_of_row=one, n_pools=0) == 0


# ------------------------------------------------------------------------------ planning
def test_plan_call():
    assert diverse.default_candidates(30, 512) == 120 and diverse.default_candidates(5, 512) == 64
    assert diverse.default_candidates(0, 512) == 64 and diverse.default_candidates(200, 512) == 512
    amount, lam, M, A = diverse.plan_call(30, 0.7, None, 512)
    assert (amount, M, A) == (30, 120, 30) and type(lam) is f32 and lam == f32(0.7)
    assert diverse.plan_call(0, 1, 5, 512)[2:] == (5, 1)            # amount 0 counts as 1
    assert diverse.plan_call(70, 0, 65, 512)[2:] == (65, 65)        # no row picks more than its candidates
    assert diverse.plan_call(np.int64(512), np.float64(0.25), 512, 512)[1:] == (f32(0.25), 512, 512)
    for trade in (-0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='trade'):
            diverse.plan_call(30, trade, None, 512)
    for cand in (0, -3):
        with pytest.raises(ValueError, match='at least 1'):
            diverse.plan_call(30, 0.7, cand, 512)
    with pytest.raises(ValueError, match='above cc_recommend_diverse_max_candidates'):
        diverse.plan_call(30, 0.7, 513, 512)


def test_check_table():
    assert [diverse.k_pad(K) for K in (1, 32, 33, 40, 64, 65, 96)] == [32, 32, 64, 64, 64, 96, 96]
    assert diverse.check_table((100, 64), 100, 512, 512) == 64
    assert diverse.check_table((100, 40), 100, 512, 512) == 40
    assert diverse.check_table((100, 96), 100, 341, 512) == 96
    assert diverse.check_table((100, 16), 100, 512, 512) == 16
    with pytest.raises(ValueError, match='at most 341'):
        diverse.check_table((100, 96), 100, 342, 512)
    with pytest.raises(ValueError, match='do not fit'):
        diverse.check_table((100, 65), 100, 512, 512)
    for shape in ((99, 64), (100,), (100, 64, 1), (100, 0)):
        with pytest.raises(ValueError, match='emb has shape'):
            diverse.check_table(shape, 100, 64, 512)


class NoLaunch:
    """What recommend_diverse_many reads off a Recommender before it launches anything."""
    V, d, dev, stream, params = 50, 64, 'cuda', None, None


def test_bad_arguments_raise_before_any_launch():
    cubes = [[1, 2, 2], [7]]
    before = [list(c) for c in cubes]
    emb = np.zeros((50, 64), f32)
    call = lambda *a, **kw: diverse.recommend_diverse_many(NoLaunch(), *a, **kw)     # noqa: E731
    for bad in ([[1, 50]], [[-1]], [[1], [2, 99]]):
        with pytest.raises(ValueError, match='outside'):
            call(bad, 10, emb=emb)
    with pytest.raises(ValueError, match='built for 60 cards'):
        call(cubes, 10, pool=CardPool([1, 2], 60), emb=emb)
    with pytest.raises(ValueError, match='1 pools for 2 cubes'):
        call(cubes, 10, pool=[CardPool([1], 50)], emb=emb)
    with pytest.raises(ValueError, match='trade'):
        call(cubes, 10, trade=1.2, emb=emb)
    with pytest.raises(ValueError, match='candidates'):
        call(cubes, 10, candidates=L.lib().cc_recommend_diverse_max_candidates() + 1, emb=emb)
    with pytest.raises(ValueError, match='candidates'):
        call(cubes, 10, candidates=0, emb=emb)
    with pytest.raises(ValueError, match='emb has shape'):
        call(cubes, 10, emb=np.zeros((49, 64), f32))
    with pytest.raises(ValueError, match='do not fit'):
        call(cubes, 10, candidates=400, emb=np.zeros((50, 96), f32))
    assert call([], 10) == [] and call([], 10, emb=emb) == []
    assert cubes == before


# ------------------------------------------------------------------------------ api and CLI
class StubModel:
    def __init__(self, out):
        self.out, self.calls = out, []

    def recommender(self):
        return self

    def recommend_diverse(self, cube, amount, trade=0.7, candidates=None, pool=None):
        self.calls.append((list(cube), amount, trade, candidates, pool))
        return self.out


def test_api_recommend_diverse_on_a_stub():
    model = StubModel({'additions': np.array([7, 3, 9], np.int32), 'add_vals': np.array([.5, .75, .25], f32),
                       'redundancy': np.array([0, .125, .5], f32), 'base_rank': np.array([1, 0, 4], np.int32),
                       'cut_vals': np.zeros(3, f32)})
    names = {i: f'card {i}' for i in range(20)}
    cube = [1, 4, 4]
    got = api.recommend_diverse(model, iter(cube), 3, names, trade=0.25, candidates=9)
    assert list(got) == ['additions', 'redundancy', 'base_rank']
    assert list(got['additions'].items()) == [('card 7', .5), ('card 3', .75), ('card 9', .25)]       # pick order
    assert list(got['redundancy'].items()) == [('card 7', 0.0), ('card 3', .125), ('card 9', .5)]
    assert list(got['base_rank'].items()) == [('card 7', 1), ('card 3', 0), ('card 9', 4)]
    assert all(type(v) is float for v in got['redundancy'].values())
    assert all(type(v) is int for v in got['base_rank'].values())
    assert model.calls == [(cube, 3, 0.25, 9, None)]


def test_cli_arguments():
    sys.path.insert(0, ROOT)
    from scripts import recommend_diverse
    a = recommend_diverse.parse_args(['my cube', '30'])
    assert (a.cube, a.amount, a.trade, a.candidates, a.pool, a.root) == ('my cube', 30, 0.7, None, None,
                                                                         'https://cubecobra.com')
    assert (a.model_dir, a.id_map) == ('ml_files/neg', 'ml_files/recommender_id_map.json')
    a = recommend_diverse.parse_args(['list.txt', '50', '--pool', 'owned.txt', '--trade', '0.4', '--candidates', '300'])
    assert (a.cube, a.amount, a.pool, a.trade, a.candidates) == ('list.txt', 50, 'owned.txt', 0.4, 300)
    for bad in ([], ['c'], ['c', 'many'], ['c', '3', '--trade', 'x']):
        with pytest.raises(SystemExit):
            recommend_diverse.parse_args(bad)
