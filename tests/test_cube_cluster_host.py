"""CPU tests of the cube archetypes' host side: the reference (tests/cube_cluster_ref.py) against a
float64 restatement, its changed / n_iter bookkeeping, the bindings against the header, the
workspace bound, every argument check of cc_cube_cluster and cc_cube_assign with never-dereferenced
pointers, CubeIndex.cluster's own checks with the library replaced by a stub, the CLI's arguments,
and that every convergence case of the GPU tests converges in the reference below its max_iter."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import cubecluster, cubesim
from tests import cube_cluster_ref as R
from tests import test_gpu_cube_cluster as G
from tests.test_cube_index_host import NoRecommender, header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'cc_cube_cluster_block': 0, 'cc_cube_cluster_max_k': 0, 'cc_cube_cluster_ws_size': 4, 'cc_cube_cluster': 15,
       'cc_cube_assign': 13}


def test_signatures_match_the_header():
    i32, P, SZ = C.c_int32, C.c_void_p, C.c_size_t
    assert L.SIGNATURES['cc_cube_cluster_ws_size'] == (SZ, [i32, i32, i32, i32])
    assert L.SIGNATURES['cc_cube_cluster'] == (C.c_int, [P, i32, i32, i32, i32, P, i32, P, P, P, P, P, P, P, P])
    assert L.SIGNATURES['cc_cube_assign'] == (C.c_int, [P, i32, i32, i32, i32, P, i32, P, P, P, P, P, P])
    lib = L.lib()
    for name, count in NEW.items():
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):       # a pointer where the header has one
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert int(lib.cc_cube_cluster_block()) == R.block() == 256 and int(lib.cc_cube_cluster_max_k()) >= 1024


def test_workspace_bound():
    """At or below 2 N Kp 4 + N k / 64 + 64 k Kp bytes plus 1 MiB: no [N][k] matrix of elements
    wider than 2 bytes fits in that (the bench shapes, and around the kernels' edges)."""
    ws = lambda N, K, k, Q: int(L.lib().cc_cube_cluster_ws_size(N, K, k, Q))   # noqa: E731
    for N, K, k in ((65536, 64, 256), (1 << 20, 64, 1024), (2504, 64, 130), (257, 70, 65), (1, 5, 1), (1 << 22, 64, 1024)):
        Kp = -(-K // 32) * 32
        got = ws(N, K, k, 0)
        assert 0 < got <= 2 * N * Kp * 4 + N * k // 64 + 64 * k * Kp + (1 << 20), (N, K, k)
        assert got % 256 == 0
        assert got < N * k * 4 or N * k * 4 < (1 << 21), (N, K, k)       # below an fp32 [N][k]
        blocks = -(-N // 256)
        assert got >= blocks * 256 * Kp * 4 + blocks * k * 2 + Kp * k * 4 + N * 8   # partials, map, image, composites
    # monotone in every argument a caller grows a kept buffer by; the query part grows with Q alone
    for name, values in dict(N=(0, 1, 255, 256, 257, 70000), K=(1, 32, 33, 64, 70), k=(1, 64, 65, 1024),
                             Q=(0, 1, 130, 4096)).items():
        base = dict(N=5000, K=64, k=130, Q=64)
        sizes = [ws(*{**base, name: v}.values()) for v in values]
        assert sizes == sorted(sizes), name
    assert ws(0, 64, 130, 4096) - ws(0, 64, 130, 0) <= 4096 * (65 * 4 + 8) + 768     # rows, flags, composites


# ------------------------------------------------------------------ the reference against float64
def f64_rows(e):
    e = np.asarray(e, np.float64)
    return e / np.sqrt(np.maximum((e * e).sum(1, keepdims=True), 1e-12))


@pytest.mark.parametrize('kind', ['relu', 'signed', 'planted', 'zero-rows'])
def test_reference_against_float64(kind):
    N, K, k = 1029, 64, 17
    e, _ = R.make_emb(kind, N, K, seed=3)
    n = R.normalise(e)
    assert np.abs(n - f64_rows(e)).max() <= K * 2.0 ** -23
    c = n[R.init_ids(N, k, seed=4)]
    B = R.block()
    for _ in range(3):
        label, dist = R.assign(n, c)
        d64 = -(n.astype(np.float64) @ c.astype(np.float64).T)
        two = np.sort(d64, axis=1)[:, :2]
        clear = (two[:, 1] - two[:, 0]) > 2.0 ** -20
        assert clear.sum() > N // 2
        assert np.array_equal(label[clear], np.argmin(d64, axis=1)[clear])
        assert np.abs(dist - d64[np.arange(N), label]).max() <= K * 2.0 ** -23
        new = R.update(n, label, c, B)
        want = c.astype(np.float64).copy()
        for j in range(k):
            if (label == j).any():
                want[j] = f64_rows(n[label == j].astype(np.float64).sum(0)[None])[0]
        assert np.abs(new - want).max() <= K * 2.0 ** -23
        empty = np.bincount(label, minlength=k) == 0
        assert np.array_equal(R.u32(new[empty]), R.u32(c[empty]))       # kept bits
        norms = np.sqrt((new[~empty].astype(np.float64) ** 2).sum(1))
        live = np.abs(want[~empty]).sum(1) > 0
        assert np.abs(norms[live] - 1).max() <= K * 2.0 ** -23
        c = new


def test_reference_ties_go_to_the_lower_centroid_and_empty_clusters_keep_their_bits():
    e, special = R.make_emb('dups', 300, 64, seed=2)
    n = R.normalise(e)
    init = np.array([10, 11, 200], np.int32)                       # rows 10 and 11 are equal
    out = R.cluster(n, init, 0)                                    # every distance to both is equal
    assert not np.any(out['label'] == 1) and out['sizes'][1] == 0 and out['sizes'][0] > 0
    out = R.cluster(n, init, 1)                                    # the empty one keeps its bits, the other moves
    assert np.array_equal(R.u32(out['centroids'][1]), R.u32(n[11]))
    assert not np.array_equal(R.u32(out['centroids'][0]), R.u32(n[10]))
    zero = R.cluster(R.normalise(np.zeros((70, 64), np.float32)), np.array([3, 4, 5]), 50)
    assert np.all(zero['label'] == 0) and np.all(R.u32(zero['dist']) == 0x80000000)
    assert zero['sizes'].tolist() == [70, 0, 0] and zero['n_iter'] == 1 and zero['changed'][:2].tolist() == [70, 0]


def test_reference_bookkeeping():
    N, K, k = 300, 64, 5
    e, _ = R.make_emb('relu', N, K, seed=1)
    n = R.normalise(e)
    init = R.init_ids(N, k, seed=1)
    full = R.cluster(n, init, 50)
    it = full['n_iter']
    assert full['converged'] and 1 <= it < 50
    assert full['changed'][0] == N and full['changed'][it] == 0 and np.all(full['changed'][:it] > 0)
    assert np.all(full['changed'][it + 1:] == -1) and len(full['changed']) == 51
    zero = R.cluster(n, init, 0)                                   # one assign with the start centroids
    assert zero['n_iter'] == 0 and zero['changed'].tolist() == [N] and not zero['converged']
    assert np.array_equal(R.u32(zero['centroids']), R.u32(n[init]))
    assert np.array_equal(zero['label'], R.assign(n, n[init])[0])
    one = R.cluster(n, init, 1)                                    # one update, then the last assign
    assert one['n_iter'] == 1 and one['changed'].tolist() == [N, int(full['changed'][1])] and not one['converged']
    assert np.array_equal(R.u32(one['centroids']), R.u32(R.update(n, zero['label'], n[init], R.block())))
    # max_iter beyond convergence changes nothing but the -1 tail; exactly at it: the last assign sees no change
    for max_iter in (it, it + 1, it + 7):
        got = R.cluster(n, init, max_iter)
        assert got['n_iter'] == it and got['converged'] and got['changed'][:it + 1].tolist() == full['changed'][:it + 1].tolist()
        assert np.all(got['changed'][it + 1:] == -1)
        for f in ('label', 'dist', 'centroids', 'sizes'):
            assert np.array_equal(R.u32(got[f]), R.u32(full[f])), f
    short = R.cluster(n, init, it - 1) if it > 1 else None
    if short is not None:
        assert short['n_iter'] == it - 1 and not short['converged'] and short['changed'][-1] > 0
    for out in (full, zero, one):                                  # labels are the assign of the returned centroids
        lab, dist = R.assign(n, out['centroids'])
        assert np.array_equal(lab, out['label']) and np.array_equal(R.u32(dist), R.u32(out['dist']))
        assert out['sizes'].sum() == N and np.array_equal(out['sizes'], np.bincount(out['label'], minlength=k))


def test_gpu_convergence_cases_converge_in_the_reference():
    """The shapes, kinds and seeds of tests/test_gpu_cube_cluster.py that run to max_iter = 50."""
    for N in G.n_values():
        n = R.normalise(R.make_emb('relu', N, 64, seed=N)[0])
        for k in G.ks_of(N):
            out = R.cluster(n, R.init_ids(N, k, seed=N + k), 50)
            assert out['converged'] and out['n_iter'] < 50, (N, k)
    for kind in R.KINDS:
        n = R.normalise(R.make_emb(kind, 1029, 64, seed=7 * R.KINDS.index(kind) + 3)[0])
        for k in (2, 65, 130):
            init = R.init_ids(1029, k, seed=k)
            if kind == 'dups':
                init[:2] = (10, 11)
            out = R.cluster(n, init, 50)
            assert out['converged'] and out['n_iter'] < 50, (kind, k)
            if kind == 'planted' and k == 130:
                assert (out['sizes'] == 0).any()


# ------------------------------------------------------------------ argument checks
def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    cap = int(lib.cc_cube_cluster_max_k())

    def run(index=one, cap_=700, N=300, K=64, k=5, init=one, max_iter=3, ws=one, label=one, dist=one, cent=one,
            sizes=one, changed=one, n_iter=one):
        return lib.cc_cube_cluster(index, cap_, N, K, k, init, max_iter, ws, label, dist, cent, sizes, changed, n_iter,
                                   None)

    def failed(entry, what):
        msg = lib.cc_last_error_string()
        return entry in msg and what in msg
    bad = [(dict(index=None), b'null'), (dict(init=None), b'null'), (dict(ws=None), b'null'), (dict(label=None), b'null'),
           (dict(dist=None), b'null'), (dict(cent=None), b'null'), (dict(sizes=None), b'null'),
           (dict(changed=None), b'null'), (dict(n_iter=None), b'null'), (dict(k=0), b'k must be'),
           (dict(k=-3), b'k must be'), (dict(k=cap + 1, N=cap + 5, cap_=cap + 5), b'k must be'), (dict(k=301), b'at most N'),
           (dict(max_iter=-1), b'max_iter'), (dict(N=-1), b'N must be'), (dict(N=701), b'N must be'),
           (dict(K=0), b'cap/K'), (dict(K=-2), b'cap/K'), (dict(cap_=0, N=0), b'cap/K'),
           (dict(ws=C.c_void_p(4096 + 8)), b'aligned'), (dict(index=C.c_void_p(4096 + 64)), b'aligned')]
    for kw, what in bad:
        assert run(**kw) == -1 and failed(b'cc_cube_cluster', what), kw
    assert run(N=0) == 0 and run(N=0, max_iter=0, k=cap) == 0      # nothing launched

    def assign(index=one, cap_=700, N=300, K=64, k=5, cent=one, Q=2, qid=one, zq=None, ws=one, label=one, dist=one):
        return lib.cc_cube_assign(index, cap_, N, K, k, cent, Q, qid, zq, ws, label, dist, None)
    bad = [(dict(index=None), b'null'), (dict(cent=None), b'null'), (dict(ws=None), b'null'), (dict(label=None), b'null'),
           (dict(dist=None), b'null'), (dict(k=0), b'k must be'), (dict(k=cap + 1), b'k must be'),
           (dict(N=-1), b'N must be'), (dict(N=701), b'N must be'), (dict(K=0), b'cap/K'), (dict(cap_=0), b'cap/K'),
           (dict(Q=-1), b'Q'), (dict(Q=(1 << 22) + 1), b'Q'), (dict(ws=C.c_void_p(4096 + 128)), b'aligned'),
           (dict(index=C.c_void_p(4096 + 8)), b'aligned')]
    for kw, what in bad:
        assert assign(**kw) == -1 and failed(b'cc_cube_assign', what), kw
        if 'Q' not in kw:                        # a failing call with no rows still fails
            assert assign(**kw, Q=0) == -1 and failed(b'cc_cube_assign', what), kw
    assert assign(Q=0) == 0 and assign(Q=0, qid=None, zq=one, k=cap) == 0 and assign(Q=0, N=0) == 0


class Stub:
    """Stands in for the _lib module: the caps may be asked for, every other use of the library is
    recorded and fails."""

    def __init__(self):
        self.calls = []

    def lib(self):
        return self

    def cc_cube_cluster_max_k(self):
        return 1024

    def cc_cube_neighbours_max_k(self):
        return 1024

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            raise AssertionError(f'the library was used: {name}')
        return record


def stub_index(monkeypatch, N, capacity):
    stub = Stub()
    monkeypatch.setattr(cubesim, 'L', stub)
    monkeypatch.setattr(cubecluster, 'L', stub)
    index = cubesim.CubeIndex(NoRecommender(), capacity=capacity)
    index.N = N                                  # as if N cubes had been put
    return index, stub


def test_cluster_checks_before_any_library_call(monkeypatch):
    index, stub = stub_index(monkeypatch, N=10, capacity=2000)
    for kw, what in ((dict(k=0), 'below 1'), (dict(k=-2), 'below 1'), (dict(k=11), 'above the 10 cubes'),
                     (dict(k=3, max_iter=-1), 'max_iter'), (dict(k=3, n_init=0), 'n_init'),
                     (dict(k=3, init=[1, 2]), 'not k = 3'), (dict(k=3, init=[1, 2, 10]), r'init 2.*outside \[0, 10\)'),
                     (dict(k=2, init=[-1, 2]), r'init 0.*outside')):
        with pytest.raises(ValueError, match=what):
            index.cluster(**kw)
    index.N = 1500
    with pytest.raises(ValueError, match=r'1025.*cc_cube_cluster_max_k\(\) = 1024'):
        index.cluster(1025)
    empty, stub2 = stub_index(monkeypatch, N=0, capacity=4)
    with pytest.raises(ValueError, match='above the 0 cubes'):
        empty.cluster(1)
    # a result's own checks
    index.N = 10
    labels = np.array([0, 1, 1, 0, 2, 1, 0, 0, 1, 1], np.int32)
    dists = -np.array([.5, .9, .9, .7, 1, .2, .7, .1, .95, .9], np.float32)
    got = cubecluster.CubeClusters(index, np.arange(4), labels, dists, None, np.zeros((4, 64), np.float32),
                                   np.bincount(labels, minlength=4).astype(np.int32), np.array([10, 0, -1], np.int32), 1)
    assert got.k == 4 and got.N == 10 and got.converged and got.n_iter == 1
    assert got.objective == pytest.approx(float(-dists.astype(np.float64).mean()), abs=0)
    assert got.members(1).tolist() == [1, 2, 5, 8, 9] and got.members(3).tolist() == []
    assert got.representatives(1, 3).tolist() == [8, 1, 2] and got.representatives(1, 99).tolist() == [8, 1, 2, 9, 5]
    assert got.representatives(0, 2).tolist() == [3, 6] and got.representatives(3, 5).tolist() == []
    for bad in (-1, 4):
        with pytest.raises(ValueError, match='cluster'):
            got.members(bad)
    for bad in ([10], [-1], [0, 11]):
        with pytest.raises(ValueError, match='outside'):
            got.predict(bad)
    with pytest.raises(ValueError, match='outside'):
        got.predict_cubes([[1, 50]])
    assert got.predict([])[0].shape == (0,) and got.predict_cubes([])[1].dtype == np.float32
    assert stub.calls == [] and stub2.calls == []


def test_initial_ids_are_the_documented_draw():
    for seed, r in ((0, 0), (5, 2)):
        want = np.random.default_rng(seed + r).choice(700, 9, replace=False)
        assert cubecluster.initial_ids(700, 9, seed, r).tolist() == want.tolist()
        assert R.init_ids(700, 9, seed + r).tolist() == want.tolist()


def test_cube_clusters_report_on_the_host():
    """api.cube_clusters's host part (the report of a finished clustering)."""
    from cubecobrarecommender_amd import api
    labels = np.array([0, 1, 1, 0, 1], np.int32)
    dists = -np.array([.5, .9, .9, .7, .8], np.float32)
    res = cubecluster.CubeClusters(None, np.arange(3), labels, dists, None, np.zeros((3, 64), np.float32),
                                   np.array([2, 3, 0], np.int32), np.array([5, 0], np.int32), 1)
    cubes = [[0, 1], [1, 2], [1, 2, 3], [0], [2]]
    rows = api.cube_clusters_report(res, cube_names=[f'c{i}' for i in range(5)], cubes=cubes,
                                    int_to_card={i: f'card{i}' for i in range(4)}, top=2, representatives=2)
    assert [r['id'] for r in rows] == [0, 1, 2] and [r['size'] for r in rows] == [2, 3, 0]
    assert rows[0]['representatives'] == [('c3', pytest.approx(.7)), ('c0', pytest.approx(.5))]
    assert rows[1]['representatives'] == [('c1', pytest.approx(.9)), ('c2', pytest.approx(.9))]
    assert rows[2]['representatives'] == [] and rows[2]['cards'] == []
    # cluster 1 holds cubes 1, 2, 4: card 2 in all three (corpus share 3 / 5), card 1 in two (corpus 3 / 5)
    assert rows[1]['cards'] == [('card2', pytest.approx(1.0), pytest.approx(5 / 3)),
                                ('card1', pytest.approx(2 / 3), pytest.approx(10 / 9))]
    assert rows[0]['cards'][0] == ('card0', pytest.approx(1.0), pytest.approx(2.5))
    plain = api.cube_clusters_report(res)
    assert plain[0]['representatives'][0][0] == 3 and 'cards' not in plain[0]


def test_cli_arguments(capsys):
    sys.path.insert(0, ROOT)
    from scripts import cluster_cubes as cli
    a = cli.parse_args(['high_req', '40'])
    assert (a.name, a.k, a.out, a.seed, a.max_iter, a.n_init, a.synthetic) == ('high_req', 40, None, 0, 50, 1, None)
    assert (a.data_dir, a.out_dir) == ('./data', './ml_files')
    a = cli.parse_args(['m', '5', '--out', 't.npz', '--seed', '4', '--max-iter', '9', '--n-init', '3', '--synthetic',
                        '700', '300', '--data-dir', 'd', '--out-dir', 'o'])
    assert (a.k, a.out, a.seed, a.max_iter, a.n_init, a.synthetic, a.data_dir, a.out_dir) == \
        (5, 't.npz', 4, 9, 3, [700, 300], 'd', 'o')
    for bad in (['m'], ['m', 'five'], ['m', '5', '--synthetic', '7']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()
