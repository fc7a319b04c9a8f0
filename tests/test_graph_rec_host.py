"""CPU tests of the co-occurrence baseline's host side: the numpy statement of the pinned
definition (tests/graph_rec_ref.py) against a pure-Python loop and against the expression the
reference scripts use, the three bindings and their argument checks, the api wrappers and the
scripts on a host stand-in for GraphRecommender (nothing is fetched, nothing is launched)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api, graphrec
from cubecobrarecommender_amd.evaluate import holdout_split
from tests import graph_rec_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wild_matrix(rng, V, ld=None):
    """Normal times 2^U(-40, 40), negatives included: any other summation order changes bits."""
    ld = V if ld is None else ld
    return rng.normal(size=(V, ld)) * np.exp2(rng.uniform(-40, 40, size=(V, ld)))


def test_reference_against_a_pure_python_loop():
    rng = np.random.default_rng(1)
    for V in (1, 2, 5, 12):
        M = wild_matrix(rng, V, V + (V % 2))
        M[rng.random(M.shape) < 0.2] = -0.0
        for n in sorted({0, 1, V // 2, V - 1, V}):
            if n < 0:
                continue
            cube = np.sort(rng.choice(V, n, replace=False))
            want = []
            for j in range(V):
                acc = 0.0
                for i in cube.tolist():
                    acc = acc + (0.0 if i == j else float(M[i, j]))
                want.append(acc)
            got = G.scores(M, rng.permutation(np.concatenate([cube, cube[:2]])))   # order and duplicates do not matter
            assert np.array_equal(got.view(np.uint64), np.array(want, np.float64).view(np.uint64))
            # the rankings, spelled out pair by pair
            adds, addv = G.additions(got, cube, V)
            miss = [j for j in range(V) if j not in set(cube.tolist())]
            assert sorted(adds.tolist()) == miss
            for a, b in zip(adds[:-1], adds[1:]):
                assert (got[a], a) > (got[b], b)
            ids, vals = G.cuts(got, cube)
            assert sorted(ids.tolist()) == cube.tolist()
            for a, b in zip(ids[:-1], ids[1:]):
                assert (got[a], a) < (got[b], b)
            assert np.array_equal(vals, got[ids]) and np.array_equal(addv, got[adds])
            pos = G.positions(got, cube)
            for t in range(V):
                want_rank = -1 if t in set(cube.tolist()) else sum((got[c], c) > (got[t], t) for c in miss)
                assert pos[t] == want_rank


def test_reference_is_the_row_sequential_numpy_sum():
    """M[S].sum(axis=0) of a C-contiguous M adds row after row: the pinned order, for the cards
    outside the cube (inside it the diagonal entry differs)."""
    rng = np.random.default_rng(2)
    V = 300
    M = wild_matrix(rng, V)
    cube = np.sort(rng.choice(V, 45, replace=False))
    missing = np.setdiff1d(np.arange(V), cube)
    s = G.scores(M, cube)
    assert np.array_equal(s[missing], M[cube].sum(axis=0)[missing])


@pytest.mark.parametrize('V,n', [(63, 2), (300, 45), (1029, 360)])
def test_reference_against_the_reference_scripts_expression(V, n):
    """adj[contains][:, missing].sum(0) (and [:, contains] of a diagonal-zeroed copy) sums the same
    numbers in another order: each side rounds at most n - 1 times, so per element
    |a - b| <= 2 (n - 1) 2^-53 sum_i |M[i][j]|."""
    rng = np.random.default_rng(V)
    for M in (wild_matrix(rng, V), rng.random((V, V))):
        cube = np.sort(rng.choice(V, n, replace=False))
        vec = np.zeros(V)
        vec[cube] = 1
        contains, missing = np.where(vec == 1)[0], np.where(vec == 0)[0]
        s = G.scores(M, cube)
        bound = 2 * (n - 1) * 2.0 ** -53 * np.abs(M[contains]).sum(axis=0)
        recs = M[contains][:, missing].sum(0)
        assert np.all(np.abs(recs - s[missing]) <= bound[missing])
        Z = M.copy()
        np.fill_diagonal(Z, 0)
        cut = Z[contains][:, contains].sum(0)
        assert np.all(np.abs(cut - s[contains]) <= (2 * (n - 1) * 2.0 ** -53 * np.abs(Z[contains]).sum(axis=0))[contains])


def header_arg_count(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])


def test_lib_declares_the_entries_and_checks_arguments_without_a_gpu():
    i32, i64, P = C.c_int32, C.c_int64, C.c_void_p
    assert L.SIGNATURES['cc_graph_rec_max_amount'] == (i32, [])
    assert L.SIGNATURES['cc_graph_rec_ws_size'] == (C.c_size_t, [i32, i32, i32])
    assert L.SIGNATURES['cc_graph_rec_f64'] == (C.c_int, [P, i64, i32, i32, P, P, i32, i32, P, P, P, P, P, P, P])
    assert L.SIGNATURES['cc_graph_rec_target_ranks_f64'] == (
        C.c_int, [P, i64, i32, i32, P, P, i32, P, P, P, i32, P, P, P, P, P, P, P])
    for name, count in (('cc_graph_rec_ws_size', 3), ('cc_graph_rec_f64', 15), ('cc_graph_rec_target_ranks_f64', 18)):
        assert len(L.SIGNATURES[name][1]) == header_arg_count(name) == count
    lib = L.lib()
    assert lib.cc_abi_version() == 2
    cap = int(lib.cc_graph_rec_max_amount())
    assert cap >= 1024
    for V, R in ((1, 1), (63, 3), (22000, 512)):
        size = int(lib.cc_graph_rec_ws_size(V, R, min(V, 400)))
        assert size % 256 == 0 and size >= R * V * 8
    one = C.c_void_p(4096)                           # never dereferenced: every call fails or has R == 0
    rec, ranks = lib.cc_graph_rec_f64, lib.cc_graph_rec_target_ranks_f64

    def call_rec(adj=one, ld=63, R=2, amount=10, ws=one, n_add=one, add_vals=one, cut_vals=one, max_n=3):
        return rec(adj, ld, 63, R, one, one, max_n, amount, ws, n_add, one, add_vals, cut_vals, None, None)

    def call_ranks(adj=one, ld=63, R=2, ws=one, tgt=one, rk=one, n_cut=0, cutoffs=None, max_n=3):
        return ranks(adj, ld, 63, R, one, one, max_n, one, tgt, cutoffs, n_cut, ws, rk, one, None, one, None, None)
    for call, name in ((call_rec, b'cc_graph_rec_f64'), (call_ranks, b'cc_graph_rec_target_ranks_f64')):
        assert call(adj=None) == -1 and b'null' in lib.cc_last_error_string() and name in lib.cc_last_error_string()
        assert call(ld=62) == -1 and b'ld' in lib.cc_last_error_string() and name in lib.cc_last_error_string()
        assert call(ws=C.c_void_p(4096 + 8)) == -1 and b'aligned' in lib.cc_last_error_string()
        assert name in lib.cc_last_error_string()
        assert call(max_n=64) == -1 and b'max_n' in lib.cc_last_error_string()
        assert call(R=-1) == -1
        assert call(R=0) == 0                        # CC_OK, nothing launched
        assert call(R=0, ld=66) == 0
    assert call_rec(n_add=None) == -1 and call_rec(add_vals=None) == -1 and call_rec(cut_vals=None) == -1
    assert call_rec(amount=cap + 1) == -1 and b'cc_graph_rec_f64' in lib.cc_last_error_string()
    assert b'amount' in lib.cc_last_error_string()
    assert call_rec(amount=cap, R=0) == 0 and call_rec(amount=0, R=0) == 0
    assert call_ranks(tgt=None) == -1 and call_ranks(rk=None) == -1
    assert call_ranks(n_cut=9, cutoffs=one) == -1 and b'n_cutoffs' in lib.cc_last_error_string()
    assert b'cc_graph_rec_target_ranks_f64' in lib.cc_last_error_string()
    assert call_ranks(n_cut=2, cutoffs=None) == -1
    assert call_ranks(n_cut=8, cutoffs=one, R=0) == 0


def small_graph(V=40, seed=3):
    rng = np.random.default_rng(seed)
    M = rng.integers(0, 4, size=(V, V)).astype(np.float64) / 4.0      # many ties
    np.fill_diagonal(M, 1e30)                                          # must show up in no score
    return M


def test_simple_recs_and_cuts_wrappers(monkeypatch):
    monkeypatch.setattr(graphrec, 'GraphRecommender', G.HostGraphRecommender)
    V = 40
    M = small_graph(V)
    keep = M.copy()
    cube = np.zeros(V)
    cards = [3, 7, 8, 21, 39]
    cube[cards] = 1
    s = G.scores(M, cards)
    assert np.all(np.abs(s) < 1e6)
    recs = api.simple_recs(cube, M)
    assert isinstance(recs, list) and len(recs) == V - len(cards) and all(isinstance(i, int) for i in recs)
    assert recs == G.additions(s, cards, V)[0].tolist()
    cuts = api.simple_cuts(cube, M)
    assert cuts == G.cuts(s, cards)[0].tolist() and sorted(cuts) == cards
    assert np.array_equal(M, keep)                                     # the caller's diagonal stays
    names = {i: f'card {i}' for i in range(V)}
    assert api.simple_recs(cube, M, names) == [names[i] for i in recs]
    assert api.simple_cuts(cube, M, names) == [names[i] for i in cuts]
    # a resident recommender is used as it is
    rec = G.HostGraphRecommender(M)
    assert api.simple_recs(cube, rec) == recs and api.simple_cuts(cube, rec) == cuts
    assert [c[1] for c in rec.calls] == [[cards], [cards]]
    # the reference's own expression orders the same numbers (exact here: quarters sum exactly)
    contains, missing = np.where(cube == 1)[0], np.where(cube == 0)[0]
    ref = M[contains][:, missing].sum(0)
    assert [int(missing[i]) for i in np.argsort(ref, kind='stable')[::-1]] == recs
    out = api.graph_recommend(rec, cards + [7], 4, names)
    assert list(out['additions']) == [names[i] for i in recs[:4]]
    assert list(out['additions'].values()) == s[recs[:4]].tolist()
    assert list(out['cuts']) == [names[i] for i in cuts] and list(out['cuts'].values()) == s[cuts].tolist()


def test_recommend_many_raises_before_any_launch():
    rec = graphrec.GraphRecommender.__new__(graphrec.GraphRecommender)   # no device, no graph: nothing can launch
    rec.V = 50
    cap = int(L.lib().cc_graph_rec_max_amount())
    with pytest.raises(ValueError, match=r'cube 1.*outside'):
        rec.recommend_many([[1, 2], [3, 50]], 10)
    with pytest.raises(ValueError, match='outside'):
        rec.recommend_many([[-1]], 10)
    with pytest.raises(ValueError, match='amount'):
        rec.recommend_many([[1, 2]], cap + 1)
    with pytest.raises(ValueError, match='outside'):
        rec.target_ranks([[1, 2], [3]], [[4], [50]])
    with pytest.raises(ValueError, match='is in the cube'):
        rec.target_ranks([[1, 2], [3]], [[4], [3]])
    with pytest.raises(ValueError, match='cutoffs'):
        rec.target_ranks([[1]], [[2]], cutoffs=range(9))
    assert rec.recommend_many([], 10) == []
    assert rec.target_ranks([], []) == ([], [], None)


def write_site(tmp_path, V, cards):
    names = {i: f'Card {i}' for i in range(V)}
    site = tmp_path / 'site' / 'cube' / 'api' / 'cubelist'
    site.mkdir(parents=True)
    lines = [f'CARD {i}' for i in cards] + ['a custom card', f'card {cards[0]}']     # case folds; unknown skipped
    (site / 'mycube').write_text('\n'.join(lines))
    out = tmp_path / 'output'
    out.mkdir()
    np.save(out / 'full_adj_mtx.npy', small_graph(V))
    (out / 'int_to_card.json').write_text(json.dumps({str(i): n.lower() for i, n in names.items()}))
    return {i: n.lower() for i, n in names.items()}


def test_recommend_and_cut_scripts_end_to_end(monkeypatch, tmp_path, capsys):
    from scripts import cut_cards, recommend
    monkeypatch.setattr(graphrec, 'GraphRecommender', G.HostGraphRecommender)
    V, cards = 40, [3, 7, 8, 21, 39]
    names = write_site(tmp_path, V, cards)
    fetched = []
    real_fetch = api.fetch_cube_list

    def fetch(cube_name, root=api.ROOT):
        fetched.append((cube_name, root))
        return real_fetch(cube_name, str(tmp_path / 'site'))           # a local directory: nothing is fetched
    monkeypatch.setattr(api, 'fetch_cube_list', fetch)
    monkeypatch.chdir(tmp_path)
    s = G.scores(small_graph(V), cards)
    adds = G.additions(s, cards, 6)[0].tolist()
    out = recommend.main(['mycube', '6'])
    assert fetched == [('mycube', api.ROOT)]
    assert list(out['additions']) == [names[i] for i in adds]
    printed = capsys.readouterr().out.split('Generating Recommendations . . . \n')[1].strip().split('\n')
    assert printed == [f'{k + 1}: {names[i]}' for k, i in enumerate(adds)]
    cut = G.cuts(s, cards)[0].tolist()
    out = cut_cards.main(['mycube', '3'])
    assert list(out['cuts']) == [names[i] for i in cut[:3]]
    printed = capsys.readouterr().out.split('Generating Recommendations . . . \n')[1].strip().split('\n')
    assert printed == [f'{k + 1}: {names[i]}' for k, i in enumerate(cut[:3])]
    assert len(cut_cards.main(['mycube'])['cuts']) == len(cards)       # fewer cards than the default 100: all of them
    assert len(recommend.main(['mycube'])['additions']) == V - len(cards)


class RanksStub:
    """target_ranks with fixed ranks: what the evaluate script needs of a model or a graph."""

    def __init__(self, rank):
        self.rank, self.calls = rank, []

    def target_ranks(self, cubes, targets, cutoffs=(), rows_per_launch=512):
        self.calls.append(([np.asarray(c) for c in cubes], [np.asarray(t) for t in targets], tuple(cutoffs)))
        return [np.full(len(t), self.rank, np.int32) for t in targets], [np.zeros(len(t)) for t in targets], None


def test_evaluate_script_baseline_sees_the_visible_cards_only(monkeypatch, capsys):
    from cubecobrarecommender_amd import model as model_mod
    from cubecobrarecommender_amd import synthetic
    from scripts import evaluate as cli
    C_, V, seed = 30, 200, 4

    def synthetic_cubes(C, V, seed=0):                                 # the real one draws on the GPU
        rng = np.random.default_rng(seed)
        lists = [np.sort(rng.choice(V, int(rng.integers(2, 40)), replace=False)).astype(np.int32) for _ in range(C)]
        return np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64), np.concatenate(lists)
    monkeypatch.setattr(synthetic, 'synthetic_cubes', synthetic_cubes)

    class Model(RanksStub):
        N = V

        def recommender(self):
            return self
    model, graph, built = Model(3), RanksStub(60), []
    monkeypatch.setattr(model_mod, 'load_model', lambda path: model)

    def from_cubes(indptr, indices, V_, device='cuda'):
        built.append((np.asarray(indptr), np.asarray(indices), V_))
        return graph
    monkeypatch.setattr(graphrec.GraphRecommender, 'from_cubes', staticmethod(from_cubes))
    argv = ['m', '10', '50', '--synthetic', str(C_), str(V), '--seed', str(seed), '--hide', '0.25']
    plain = cli.main(argv)
    plain_line = capsys.readouterr().out
    assert built == [] and 'cooccurrence' not in plain
    both = cli.main(argv + ['--baseline'])
    line = capsys.readouterr().out
    # the graph: one build, from the visible part of every cube and nothing else
    indptr, idx = synthetic_cubes(C_, V, seed=seed)
    cubes = [idx[indptr[c]:indptr[c + 1]] for c in range(C_)]
    visible, hidden = holdout_split(cubes, hide=0.25, seed=seed)
    assert len(built) == 1 and built[0][2] == V
    got_ptr, got_idx, _ = built[0]
    assert np.array_equal(got_ptr, np.concatenate([[0], np.cumsum([len(v) for v in visible])]))
    assert np.array_equal(got_idx, np.concatenate(visible))
    for c in range(C_):
        assert len(np.intersect1d(got_idx[got_ptr[c]:got_ptr[c + 1]], hidden[c])) == 0
    assert sum(len(h) for h in hidden) > 0
    # the baseline is asked about the same split with the same cut-offs
    assert len(graph.calls) == 1 and graph.calls[0][2] == (10, 50)
    for a, b in zip(graph.calls[0][0], visible):
        assert np.array_equal(a, b)
    for a, b in zip(graph.calls[0][1], hidden):
        assert np.array_equal(a, b)
    assert both['cooccurrence']['recall@10'] == 0.0 and both['cooccurrence']['recall@50'] == 0.0
    assert both['recall@10'] == 1.0 and both['cooccurrence']['n_targets'] == both['n_targets']
    # without the flag: what it printed before; with it, that plus the one block
    rest = {k: v for k, v in both.items() if k != 'cooccurrence'}
    assert rest == plain and json.dumps(rest) + '\n' == plain_line
    assert json.loads(line) == both and list(json.loads(line))[-1] == 'cooccurrence'
