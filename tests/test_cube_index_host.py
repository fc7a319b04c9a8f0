"""CPU tests of the cube index's host side: the five bindings against the header, the size
functions (the search workspace never grows with Q x N), every argument check of cc_cube_index_put
and cc_cube_neighbours with never-dereferenced pointers (each call either fails or launches
nothing), CubeIndex's own checks with the library replaced by a stub, and the CLI's arguments."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import cubesim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'cc_cube_index_size': 2, 'cc_cube_index_put': 7, 'cc_cube_neighbours_max_k': 0,
       'cc_cube_neighbours_ws_size': 5, 'cc_cube_neighbours': 14}


def header_args(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return [a.strip() for a in args.split(',') if a.strip() and a.strip() != 'void']


def test_signatures_match_the_header():
    i32, P, SZ = C.c_int32, C.c_void_p, C.c_size_t
    assert L.SIGNATURES['cc_cube_index_size'] == (SZ, [i32, i32])
    assert L.SIGNATURES['cc_cube_index_put'] == (C.c_int, [P, i32, i32, i32, i32, P, P])
    assert L.SIGNATURES['cc_cube_neighbours_max_k'] == (i32, [])
    assert L.SIGNATURES['cc_cube_neighbours_ws_size'] == (SZ, [i32, i32, i32, i32, i32])
    assert L.SIGNATURES['cc_cube_neighbours'] == (C.c_int, [P, i32, i32, i32, i32, P, P, P, i32, i32, P, P, P, P])
    lib = L.lib()
    for name, count in NEW.items():
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):       # a pointer where the header has one
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert lib.cc_abi_version() == 2


def test_workspace_never_grows_with_queries_times_corpus():
    lib = L.lib()
    ws = lambda N, K, Q, k, chunk: int(lib.cc_cube_neighbours_ws_size(N, K, Q, k, chunk))   # noqa: E731
    assert int(lib.cc_cube_neighbours_max_k()) >= 1024
    # an eighth of the 2 GiB a [Q][N] key matrix would take
    assert ws(1 << 20, 64, 512, 100, 0) < 256 << 20 == (512 * (1 << 20) * 4) // 8
    # N doubles at fixed Q, k and chunk, from one whole chunk on: the keys stay [Q][chunk] and only
    # the candidates grow, by Q * k * 8 bytes per added chunk (and one 256-byte rounding)
    for Q, k, chunk, first in ((512, 100, 0, 1 << 16), (512, 40, 1024, 1024), (7, 1024, 64, 64), (130, 1, 4096, 4096)):
        step = chunk or first                                      # chunk 0: the default, `first` cubes
        N = first
        while N < (1 << 22):
            grown, added_chunks = ws(2 * N, 64, Q, k, chunk) - ws(N, 64, Q, k, chunk), N // step
            assert 0 < grown <= added_chunks * Q * k * 8 + 256, (Q, k, chunk, N)
            N *= 2
    # below one chunk the keys are [Q][N rounded up to 64]: never more than [Q][chunk]
    for chunk in (64, 1024, 0):
        whole = chunk or (1 << 16)
        for N in (1, 63, 64, 65, 300, 1000):
            if N <= whole:
                assert ws(N, 64, 512, 40, chunk) <= ws(whole, 64, 512, 40, chunk), (N, chunk)


def test_size_functions_are_monotone_and_256_byte_multiples():
    """Monotone in every argument the callers grow a kept buffer by (N, K, Q, k; cap and K of the
    index).  chunk trades the key term (Q * min(chunk, N), rising) against the candidate term
    (Q * k * ceil(N / chunk), falling), so it is held to those two terms instead."""
    lib = L.lib()
    ws = lambda *a: int(lib.cc_cube_neighbours_ws_size(*a))        # noqa: E731
    ix = lambda *a: int(lib.cc_cube_index_size(*a))                # noqa: E731
    base = dict(N=5000, K=64, Q=130, k=40, chunk=1024)
    steps = dict(N=(1, 63, 64, 65, 1024, 1025, 5000, 70000, 1 << 20), K=(1, 5, 32, 33, 64, 70, 256),
                 Q=(1, 7, 32, 33, 64, 65, 130, 512, 4096), k=(1, 2, 40, 100, 1024))
    for name, values in steps.items():
        for chunk in (64, 1024, 0):
            sizes = [ws(*{**base, 'chunk': chunk, name: v}.values()) for v in values]
            assert sizes == sorted(sizes) and all(s % 256 == 0 and s > 0 for s in sizes), (name, chunk)
    for chunk in (64, 128, 1024, 65536, 0):
        N, K, Q, k = 5000, 64, 130, 40
        eff = chunk or 65536
        keys, cand = Q * min(eff, -(-N // 64) * 64) * 4, Q * k * -(-N // eff) * 8
        fixed = Q * 64 * 4 + Q * 4                                 # the queries' rows and flags
        assert keys + cand + fixed <= ws(N, K, Q, k, chunk) <= keys + cand + fixed + 5 * 256
    caps, Ks = (1, 63, 64, 65, 700, 65536, 1 << 20), (1, 5, 32, 33, 64, 70)
    for K in Ks:
        sizes = [ix(cap, K) for cap in caps]
        assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
        assert all(s >= 2 * cap * K * 4 for s, cap in zip(sizes, caps))     # n and nT
    for cap in caps:
        sizes = [ix(cap, K) for K in Ks]
        assert sizes == sorted(sizes)
    assert ix(1 << 20, 64) <= 2 * (1 << 20) * 64 * 4 + 512          # K = 64, cap a multiple of 64: no pad


def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    cap = int(lib.cc_cube_neighbours_max_k())

    def search(index=one, cap_=700, N=300, K=64, Q=2, qid=one, zq=None, skip=None, k=10, chunk=0, ws=one,
               out_idx=one, out_dist=one):
        return lib.cc_cube_neighbours(index, cap_, N, K, Q, qid, zq, skip, k, chunk, ws, out_idx, out_dist, None)

    def failed(entry, what):
        msg = lib.cc_last_error_string()
        return entry in msg and what in msg
    bad = [(dict(index=None), b'null'), (dict(ws=None), b'null'), (dict(out_idx=None), b'null'),
           (dict(out_dist=None), b'null'), (dict(k=0), b'k must be'), (dict(k=-2), b'k must be'),
           (dict(k=cap + 1), b'k must be'), (dict(N=0), b'N must be'), (dict(N=-1), b'N must be'),
           (dict(N=701), b'N must be'), (dict(K=0), b'cap/K'), (dict(K=-3), b'cap/K'), (dict(cap_=0, N=1), b'cap/K'),
           (dict(chunk=-64), b'chunk'), (dict(chunk=1), b'chunk'), (dict(chunk=65), b'chunk'), (dict(chunk=96), b'chunk'),
           (dict(ws=C.c_void_p(4096 + 8)), b'aligned'), (dict(ws=C.c_void_p(4096 + 128)), b'aligned'),
           (dict(index=C.c_void_p(4096 + 64)), b'aligned'), (dict(Q=-1), b'Q'), (dict(Q=(1 << 22) + 1), b'Q')]
    for kw, what in bad:
        assert search(**kw) == -1 and failed(b'cc_cube_neighbours', what), kw
        if 'Q' not in kw:                        # a failing call with no rows still fails
            assert search(**kw, Q=0) == -1 and failed(b'cc_cube_neighbours', what), kw
    # Q == 0: CC_OK, nothing launched; the optional pointers may all be absent
    assert search(Q=0) == 0 and search(Q=0, qid=None) == 0 and search(Q=0, zq=one, skip=one, k=cap, chunk=64) == 0
    assert search(Q=0, N=700, cap_=700) == 0 and search(Q=0, N=1, cap_=1, K=1, k=1) == 0

    def put(index=one, cap_=700, K=64, n0=0, rows=8, z=one):
        return lib.cc_cube_index_put(index, cap_, K, n0, rows, z, None)
    bad = [(dict(index=None), b'null'), (dict(z=None), b'null'), (dict(index=C.c_void_p(4096 + 8)), b'aligned'),
           (dict(cap_=0), b'cap/K'), (dict(K=0), b'cap/K'), (dict(n0=-1), b'inside'), (dict(rows=-1), b'inside'),
           (dict(n0=693), b'inside'), (dict(n0=700, rows=1), b'inside'), (dict(n0=2**31 - 1, rows=2**31 - 1), b'inside')]
    for kw, what in bad:
        assert put(**kw) == -1 and failed(b'cc_cube_index_put', what), kw
    # rows == 0: CC_OK, nothing launched, anywhere inside the capacity
    assert put(rows=0) == 0 and put(rows=0, n0=700) == 0 and put(rows=0, n0=123) == 0
    assert put(rows=0, n0=701) == -1 and failed(b'cc_cube_index_put', b'inside')


class Stub:
    """Stands in for the _lib module inside cubesim: the cap may be asked for, every other use of
    the library is recorded and fails."""

    def __init__(self, cap=1024):
        self.calls, self.cap = [], cap

    def lib(self):
        return self

    def cc_cube_neighbours_max_k(self):
        return self.cap

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            raise AssertionError(f'the library was used: {name}')
        return record


class NoRecommender:
    """What CubeIndex reads off a Recommender before it launches anything."""
    V, d, dev, stream, params = 50, 64, 'cuda', None, None


def empty_index(monkeypatch, N=0, capacity=None):
    stub = Stub()
    monkeypatch.setattr(cubesim, 'L', stub)
    index = cubesim.CubeIndex(NoRecommender(), capacity=capacity)
    index.N = N                                  # as if N cubes had been put
    return index, stub


def test_construction_and_add_check_before_any_library_call(monkeypatch):
    index, stub = empty_index(monkeypatch)
    assert len(index) == 0 and index.capacity == 1            # at least 1
    assert empty_index(monkeypatch, capacity=7)[0].capacity == 7
    for capacity in (0, -1):
        with pytest.raises(ValueError, match='capacity'):
            cubesim.CubeIndex(NoRecommender(), capacity=capacity)
    for bad in ([[1, 2], [3, 50]], [[-1]], [[], [0, 10**6]]):
        with pytest.raises(ValueError, match=r'cube 1|cube 0'):
            cubesim.CubeIndex(NoRecommender(), bad)
        with pytest.raises(ValueError, match='outside'):
            index.add(bad)
        with pytest.raises(ValueError, match='outside'):
            index.neighbours_of(bad, 5)
    with pytest.raises(ValueError, match='capacity'):         # three cubes into a capacity of two
        cubesim.CubeIndex(NoRecommender(), [[1], [2], [3]], capacity=2)
    index, stub = empty_index(monkeypatch, N=5, capacity=6)
    with pytest.raises(ValueError, match='capacity 6'):
        index.add([[1], [2]])
    assert index.add([]) == range(5, 5) and len(index) == 5
    model = type('Model', (), {'recommender': lambda self: NoRecommender()})()
    assert cubesim.CubeIndex(model, capacity=3).V == 50        # a model or its recommender
    assert stub.calls == []


def test_neighbours_check_ids_and_k_before_any_library_call(monkeypatch):
    index, stub = empty_index(monkeypatch, N=10, capacity=16)
    for bad in ([3, 10], [-1], [0, 1, 10**6], np.array([9, 10])):
        with pytest.raises(ValueError, match='outside'):
            index.neighbours(bad, 5)
    with pytest.raises(ValueError, match=r'query 1.*10'):
        index.neighbours([3, 10, -1], 5)
    with pytest.raises(ValueError, match='outside'):          # the id check comes first, whatever k is
        index.neighbours([10], 0)
    for call in (lambda k: index.neighbours([1], k), lambda k: index.neighbours_of([[1]], k),
                 lambda k: index.table(k)):
        with pytest.raises(ValueError, match=r'1025.*cc_cube_neighbours_max_k\(\) = 1024'):
            call(1025)
    for chunk in (-64, 1, 96):
        with pytest.raises(ValueError, match='chunk'):
            index.neighbours([1], 5, chunk=chunk)
    assert stub.calls == []


def test_empty_results_need_no_launch(monkeypatch):
    index, stub = empty_index(monkeypatch, N=10, capacity=16)
    for k in (0, -4):
        for got in (index.neighbours([1, 2, 2], k), index.neighbours_of([[1], [2, 3], []], k)):
            assert got[0].shape == (3, 0) and got[0].dtype == np.int32
            assert got[1].shape == (3, 0) and got[1].dtype == np.float32
        assert index.table(k)[0].shape == (10, 0)
    idx, dist = index.neighbours([], 7)
    assert idx.shape == (0, 7) and dist.shape == (0, 7) and idx.dtype == np.int32 and dist.dtype == np.float32
    assert index.neighbours([], 80)[0].shape == (0, 9)         # n = min(k, N - 1) without the cube itself
    assert index.neighbours([], 80, exclude_self=False)[0].shape == (0, 10)
    assert index.neighbours_of([], 80)[0].shape == (0, 10)
    one, _ = empty_index(monkeypatch, N=1, capacity=1)
    assert one.neighbours([0, 0], 5)[0].shape == (2, 0)        # nothing but the cube itself
    none, stub2 = empty_index(monkeypatch)
    assert none.neighbours_of([[1, 2]], 5)[0].shape == (1, 0) and none.table(5)[0].shape == (0, 0)
    assert stub.calls == [] and stub2.calls == []


def test_cli_arguments(capsys):
    sys.path.insert(0, ROOT)
    from scripts import similar_cubes as cli
    a = cli.parse_args(['high_req', '40', '--out', 't.npz'])
    assert (a.name, a.k, a.query, a.out, a.synthetic) == ('high_req', 40, None, 't.npz', None)
    assert (a.data_dir, a.out_dir, a.seed) == ('./data', './ml_files', 0)
    a = cli.parse_args(['m', '5', '--query', '3', '9', '3', '--synthetic', '700', '300', '--seed', '4',
                        '--data-dir', 'd', '--out-dir', 'o'])
    assert (a.k, a.query, a.out, a.synthetic, a.seed, a.data_dir, a.out_dir) == (5, [3, 9, 3], None, [700, 300], 4, 'd', 'o')
    for bad in (['m', '5'], ['m'], ['m', 'five', '--out', 'x'], ['m', '5', '--query']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()
