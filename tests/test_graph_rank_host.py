"""CPU tests of the co-occurrence baseline's full ranking, host side: the two bindings
(cc_graph_rank_ws_size, cc_graph_rank_f64) and their argument checks, GraphRecommender.rank_many's
checks before any launch, the launch cap graph_rank_rows_per_launch, and the api functions on
stand-ins for GraphRecommender (nothing is launched)."""
import ctypes as C

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api, graphrec
from tests import graph_rec_ref as G
from tests.test_graph_rec_host import header_arg_count, small_graph


def test_lib_declares_the_entries():
    i32, i64, P = C.c_int32, C.c_int64, C.c_void_p
    assert L.SIGNATURES['cc_graph_rank_ws_size'] == (C.c_size_t, [i32, i32, i32])
    assert L.SIGNATURES['cc_graph_rank_f64'] == (C.c_int, [P, i64, i32, i32, P, P, i32, i32, P, P, P, P, P, P, P])
    for name, count in (('cc_graph_rank_ws_size', 3), ('cc_graph_rank_f64', 15)):
        assert len(L.SIGNATURES[name][1]) == header_arg_count(name) == count
    assert L.lib().cc_abi_version() == 2


def test_argument_checks_without_a_gpu():
    lib = L.lib()
    cap = int(lib.cc_graph_rec_max_amount())
    one = C.c_void_p(4096)                           # never dereferenced: every call fails or has R == 0
    name = b'cc_graph_rank_f64'

    def call(adj=one, ld=63, R=2, amount=10, ws=one, n_add=one, additions=one, add_vals=one, cut_vals=one, max_n=3):
        return lib.cc_graph_rank_f64(adj, ld, 63, R, one, one, max_n, amount, ws, n_add, additions, add_vals,
                                     cut_vals, None, None)
    for kw in (dict(adj=None), dict(ws=None), dict(n_add=None), dict(additions=None), dict(cut_vals=None)):
        assert call(**kw) == -1, kw
        assert b'null' in lib.cc_last_error_string() and name in lib.cc_last_error_string(), kw
    assert call(ld=62) == -1 and b'ld' in lib.cc_last_error_string() and name in lib.cc_last_error_string()
    assert call(ws=C.c_void_p(4096 + 8)) == -1 and b'aligned' in lib.cc_last_error_string()
    assert name in lib.cc_last_error_string()
    assert call(max_n=64) == -1 and b'max_n' in lib.cc_last_error_string() and name in lib.cc_last_error_string()
    assert call(R=-1) == -1 and name in lib.cc_last_error_string()
    assert call(R=0) == 0                            # CC_OK, nothing launched
    for amount in (0, cap + 1, 2 ** 31 - 1):         # any amount is legal
        assert call(R=0, amount=amount) == 0
    assert call(R=0, add_vals=None) == 0 and call(R=0, amount=cap + 1, add_vals=None) == 0


@pytest.mark.parametrize('V,R', [(1, 1), (63, 3), (22000, 512)])
def test_workspace_size(V, R):
    lib = L.lib()
    max_n = min(V, 400)
    size = int(lib.cc_graph_rank_ws_size(V, R, max_n))
    assert size % 256 == 0
    assert size >= int(lib.cc_graph_rec_ws_size(V, R, max_n))
    assert size >= R * V * (8 + 2 * (8 + 4))         # the keys and the two (key, card) ping-pong arrays


def test_rank_many_raises_before_any_launch():
    rec = graphrec.GraphRecommender.__new__(graphrec.GraphRecommender)   # no device, no graph: nothing can launch
    rec.V = 50
    with pytest.raises(ValueError, match=r'cube 1.*outside'):
        rec.rank_many([[1, 2], [3, 50]])
    with pytest.raises(ValueError, match=r'cube 0.*outside'):
        rec.rank_many([[-1]], 10)
    assert rec.rank_many([]) == []
    assert rec.rank_many([], 10, want_vals=False, want_scores=True) == []


def test_graph_rank_rows_per_launch():
    f = graphrec.graph_rank_rows_per_launch
    assert f.__defaults__[-1] == graphrec.RANK_STAGING_BYTES

    def per_row(V, A, want_vals, want_scores):
        return 4 + 4 * A + (8 * A if want_vals else 0) + (8 * V if want_scores else 0)
    for V, A in ((1, 1), (63, 63), (22000, 100), (22000, 22000)):
        for rpl in (1, 7, 512, 100000):
            for budget in (0, 1, 1000, 1 << 20, 128 << 20):
                for wv in (True, False):
                    for ws in (True, False):
                        n = f(V, A, rpl, wv, ws, budget)
                        assert 1 <= n <= rpl
                        row = per_row(V, A, wv, ws)
                        if n > 1:
                            assert n * row <= budget
                        if n < rpl:
                            assert (n + 1) * row > budget             # one more row would not fit
    V = A = 22000
    assert per_row(V, A, True, False) == 264004                        # 264 KB a row with values
    with_vals = f(V, A, 100000)
    assert with_vals == (128 << 20) // 264004
    assert f(V, A, 100000, want_vals=False) > with_vals > f(V, A, 100000, want_scores=True)
    assert f(V, A, 512, budget_bytes=0) == 1


class RankStub:
    """A GraphRecommender stand-in that offers rank_many and recommend_many over the host
    reference and records its calls."""

    def __init__(self, M, answer=None):
        self.host = G.HostGraphRecommender(M)
        self.V = self.host.V
        self.answer, self.calls = answer, []

    def recommend_many(self, cubes, amount, want_scores=False, rows_per_launch=512):
        self.calls.append(('recommend_many', [list(map(int, c)) for c in cubes], amount))
        return self.host.recommend_many(cubes, amount, want_scores=want_scores)

    def rank_many(self, cubes, amount=None, want_vals=True, want_scores=False, rows_per_launch=512):
        self.calls.append(('rank_many', [list(map(int, c)) for c in cubes], amount, want_vals))
        if self.answer is not None:
            return [{'additions': np.asarray(self.answer, np.int32)} for _ in cubes]
        outs = self.host.recommend_many(cubes, self.V if amount is None else amount, want_scores=want_scores)
        if not want_vals:
            for o in outs:
                del o['add_vals']
        return outs


def test_simple_recs_uses_rank_many_where_it_is_offered():
    V, cards = 40, [3, 7, 8, 21, 39]
    M = small_graph(V)
    cube = np.zeros(V)
    cube[cards] = 1
    stub = RankStub(M, answer=[5, 4, 9])             # not the ranking: the stub's answer is what comes back
    assert api.simple_recs(cube, stub) == [5, 4, 9]
    assert stub.calls == [('rank_many', [cards], None, False)]
    names = {i: f'card {i}' for i in range(V)}
    assert api.simple_recs(cube, stub, names) == ['card 5', 'card 4', 'card 9']
    # the real ranking through rank_many is the list the fallback path gives
    s = G.scores(M, cards)
    want = G.additions(s, cards, V)[0].tolist()
    stub = RankStub(M)
    assert api.simple_recs(cube, stub) == want and [c[0] for c in stub.calls] == ['rank_many']


def test_simple_recs_falls_back_without_rank_many():
    V, cards = 40, [3, 7, 8, 21, 39]
    M = small_graph(V)
    cube = np.zeros(V)
    cube[cards] = 1
    rec = G.HostGraphRecommender(M)
    assert not hasattr(rec, 'rank_many')
    s = G.scores(M, cards)
    recs = api.simple_recs(cube, rec)
    assert recs == G.additions(s, cards, V)[0].tolist() and len(recs) == V - len(cards)
    assert rec.calls == [('recommend_many', [cards], 1, True)]


def test_simple_recs_many_is_a_loop_of_simple_recs():
    V = 40
    M = small_graph(V)
    rng = np.random.default_rng(5)
    cubes = [[], [0], [3, 7, 8, 21, 39, 7], list(range(V))] + [rng.choice(V, 12).tolist() for _ in range(3)]
    stub = RankStub(M)
    got = api.simple_recs_many(cubes, stub)
    assert len(stub.calls) == 1 and stub.calls[0][0] == 'rank_many'               # one call for all cubes
    assert stub.calls[0][2] is None and stub.calls[0][3] is False
    names = {i: f'card {i}' for i in range(V)}
    named = api.simple_recs_many(cubes, stub, names)
    for cards, ids, ns in zip(cubes, got, named):
        vec = np.zeros(V)
        vec[cards] = 1
        assert ids == api.simple_recs(vec, stub) == api.simple_recs(vec, G.HostGraphRecommender(M))
        assert all(isinstance(i, int) for i in ids) and ns == [names[i] for i in ids]
    assert got[3] == [] and len(got[0]) == V


def test_graph_recommend_above_the_cap_reaches_rank_many():
    V, cards = 40, [3, 7, 8, 21, 39]
    M = small_graph(V)
    names = {i: f'card {i}' for i in range(V)}
    cap = api.graph_rec_max_amount()
    assert cap == int(L.lib().cc_graph_rec_max_amount())
    s = G.scores(M, cards)
    adds, cuts = G.additions(s, cards, V)[0].tolist(), G.cuts(s, cards)[0].tolist()
    stub = RankStub(M)
    out = api.graph_recommend(stub, cards + [7], cap + 1, names)
    assert stub.calls == [('rank_many', [cards + [7]], cap + 1, True)]
    assert list(out['additions']) == [names[i] for i in adds] and list(out['additions'].values()) == s[adds].tolist()
    assert list(out['cuts']) == [names[i] for i in cuts] and list(out['cuts'].values()) == s[cuts].tolist()
    stub = RankStub(M)
    at_cap = api.graph_recommend(stub, cards + [7], cap, names)
    assert stub.calls == [('recommend_many', [cards + [7]], cap)]
    assert at_cap == out                             # V - n is below the cap here: the same complete lists
    rec = G.HostGraphRecommender(M)                  # no rank_many: the select path whatever the amount
    api.graph_recommend(rec, cards, cap + 1, names)
    assert [c[0] for c in rec.calls] == ['recommend_many']
