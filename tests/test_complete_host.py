"""CPU tests of greedy completion's host side: the three bindings against the header, the argument
checks of cc_complete_fp32 with never-dereferenced pointers, the workspace size, the host's pass
count and output pitch, the checks that come before any launch, and the CLI's arguments."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api, complete
from cubecobrarecommender_amd.complete import per_cube_sizes, plan_passes
from cubecobrarecommender_amd.recommender import CardPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_args(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return [a.strip() for a in args.split(',') if a.strip() and a.strip() != 'void']


def test_signatures_match_the_header():
    i32, P, SZ = C.c_int32, C.c_void_p, C.c_size_t
    assert L.SIGNATURES['cc_complete_max_per_step'] == (i32, [])
    assert L.SIGNATURES['cc_complete_ws_size'] == (SZ, [i32] * 5)
    assert L.SIGNATURES['cc_complete_fp32'] == (
        C.c_int, [P, i32, i32, i32, P, P, i32, P, i32, i32, P, i32, P, i32, P, P, P, P, SZ, P])
    lib = L.lib()
    for name, count in (('cc_complete_max_per_step', 0), ('cc_complete_ws_size', 5), ('cc_complete_fp32', 20)):
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):       # a pointer where the header has one
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert lib.cc_abi_version() == 2
    assert 256 <= lib.cc_complete_max_per_step() <= lib.cc_recommend_batch_max_amount()


def test_workspace_size():
    lib = L.lib()
    ws = lambda R, n, m, V=22000, d=512: int(lib.cc_complete_ws_size(V, d, R, n, m))       # noqa: E731
    base = ws(64, 360, 8)
    assert base % 256 == 0
    # the pooled select chain, then 2 CSR buffers and the cut values of R * max_n words, the picks
    chain = int(lib.cc_recommend_batch_pool_ws_size(22000, 512, 64, 360)) - 256
    own = 3 * 64 * 360 * 4 + 2 * 65 * 4 + 64 * 4 + 2 * 64 * 8 * 4
    assert chain + own <= base <= chain + own + 9 * 256
    for a, b in (((64, 360, 8), (65, 360, 8)), ((64, 360, 8), (64, 361, 8)), ((64, 360, 8), (64, 360, 9)),
                 ((1, 0, 1), (2, 0, 1)), ((1, 0, 1), (1, 33, 1)), ((512, 360, 1), (512, 360, 256))):
        assert ws(*a) <= ws(*b), (a, b)
    assert ws(64, 360, 1) < ws(64, 360, 256) and ws(64, 360, 8) < ws(512, 360, 8) and ws(64, 32, 8) < ws(64, 360, 8)
    assert ws(0, 0, 0) > 0                                          # degenerate sizes count as 1


def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    need = int(lib.cc_complete_ws_size(100, 64, 2, 40, 4))

    def call(params=one, V=100, d=64, R=2, row_ptr=one, idx=one, max_n=40, target_n=one, per_step=4, passes=3,
             pools=None, n_pools=0, pool_of_row=None, A=10, n_added=one, added=one, added_vals=one, ws=one,
             ws_bytes=need):
        return lib.cc_complete_fp32(params, V, d, R, row_ptr, idx, max_n, target_n, per_step, passes, pools, n_pools,
                                    pool_of_row, A, n_added, added, added_vals, ws, ws_bytes, None)

    def failed(what):
        msg = lib.cc_last_error_string()
        return b'cc_complete_fp32' in msg and what in msg
    top = lib.cc_complete_max_per_step()
    bad = [(dict(params=None), b'null'), (dict(row_ptr=None), b'null'), (dict(idx=None), b'null'),
           (dict(target_n=None), b'null'), (dict(n_added=None), b'null'), (dict(added=None), b'null'),
           (dict(added_vals=None), b'null'), (dict(ws=None), b'null'),
           (dict(pools=one, n_pools=1), b'null'), (dict(n_pools=1), b'null'),
           (dict(pool_of_row=one, n_pools=-1), b'n_pools'), (dict(pool_of_row=one, n_pools=2), b'pools is null'),
           (dict(d=0), b'd must be'), (dict(d=96), b'd must be'), (dict(d=2048), b'd must be'),
           (dict(max_n=101), b'max_n'), (dict(max_n=-1), b'max_n'), (dict(V=0), b'V'), (dict(R=-1), b'R'),
           (dict(A=0), b'A'), (dict(per_step=0), b'per_step'), (dict(per_step=-3), b'per_step'),
           (dict(per_step=top + 1, ws_bytes=1 << 40), b'per_step'), (dict(passes=-1), b'passes'),
           (dict(ws=C.c_void_p(4096 + 64)), b'aligned'), (dict(ws_bytes=need - 1), b'workspace'),
           (dict(ws_bytes=0), b'workspace')]
    for kw, what in bad:
        assert call(**kw) == -1 and failed(what), kw
    # R == 0 or passes == 0: CC_OK, nothing launched
    assert call(R=0) == 0 and call(passes=0) == 0 and call(R=0, passes=0) == 0
    assert call(passes=0, pool_of_row=one, n_pools=0) == 0


def test_pass_count_and_pitch():
    #                ns            sizes           m   V     target           passes  A  max_n
    cases = [([180], [360], 1, 22000, [360], 180, 180, 360),
             ([180], [360], 8, 22000, [360], 23, 180, 360),
             ([180, 10, 400], [360, 11, 100], 7, 22000, [360, 11, 100], 26, 180, 400),
             ([5, 9], [5, 3], 4, 50, [5, 3], 0, 1, 9),               # nothing to add: no pass, a pitch of 1
             ([60], [100], 4, 70, [70], 3, 10, 70),                  # the target is capped at V
             ([0], [1], 256, 10, [1], 1, 1, 1),
             ([3, 3], [-4, 10], 3, 100, [0, 10], 3, 7, 10),
             ([], [], 1, 10, [], 0, 1, 0)]
    for ns, sizes, m, V, target, passes, A, max_n in cases:
        got = plan_passes(ns, sizes, m, V)
        assert got[0].dtype == np.int32 and got[0].tolist() == target
        assert got[1:] == (passes, A, max_n), (ns, sizes, m, got)
    assert per_cube_sizes(7, 3).tolist() == [7, 7, 7] and per_cube_sizes(np.int64(7), 2).tolist() == [7, 7]
    assert per_cube_sizes([4, 5], 2).tolist() == [4, 5] and per_cube_sizes(np.array([4, 5]), 2).tolist() == [4, 5]
    with pytest.raises(ValueError, match='1 sizes for 2 cubes'):
        per_cube_sizes([4], 2)


class NoLaunch:
    """What complete_many reads off a Recommender before it launches anything."""
    V, d, dev, stream, params = 50, 64, 'cuda', None, None


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    used = []
    monkeypatch.setattr(complete.L, 'lib', lambda: used.append('lib'))
    cubes = [[1, 2, 2], [7]]
    before = [list(c) for c in cubes]
    for bad in ([[1, 50]], [[-1]], [[1], [2, 99]]):
        with pytest.raises(ValueError, match='outside'):
            complete.complete_many(NoLaunch(), bad, 10)
    with pytest.raises(ValueError, match='built for 60 cards'):
        complete.complete_many(NoLaunch(), cubes, 10, pool=CardPool([1, 2], 60))
    with pytest.raises(ValueError, match='1 pools for 2 cubes'):
        complete.complete_many(NoLaunch(), cubes, 10, pool=[CardPool([1], 50)])
    with pytest.raises(ValueError, match='3 sizes for 2 cubes'):
        complete.complete_many(NoLaunch(), cubes, [1, 2, 3])
    with pytest.raises(ValueError, match='per_step'):
        complete.complete_many(NoLaunch(), cubes, 10, per_step=0)
    assert complete.complete_many(NoLaunch(), [], 10) == [] and complete.complete_many(NoLaunch(), [], []) == []
    assert used == [] and cubes == before


class StubModel:
    def __init__(self, out):
        self.out, self.calls = out, []

    def recommender(self):
        return self

    def complete(self, cube, size, per_step=1, pool=None):
        self.calls.append((list(cube), size, per_step, pool))
        return self.out


def test_api_complete_cube_on_a_stub():
    f = np.float32
    model = StubModel({'added': np.array([7, 3, 9], np.int32), 'added_vals': np.array([.5, .75, .25], f)})
    names = {i: f'card {i}' for i in range(20)}
    cube = [1, 4, 4]
    got = api.complete_cube(model, iter(cube), 6, names, per_step=2)
    assert list(got['additions'].items()) == [('card 7', .5), ('card 3', .75), ('card 9', .25)]   # pick order
    assert model.calls == [(cube, 6, 2, None)]


def test_cli_arguments():
    sys.path.insert(0, ROOT)
    from scripts import complete_cube
    a = complete_cube.parse_args(['my cube', '360'])
    assert (a.cube, a.size, a.per_step, a.pool, a.root) == ('my cube', 360, 1, None, 'https://cubecobra.com')
    assert (a.model_dir, a.id_map) == ('ml_files/neg', 'ml_files/recommender_id_map.json')
    a = complete_cube.parse_args(['list.txt', '540', '--pool', 'owned.txt', '--per-step', '8'])
    assert (a.cube, a.size, a.pool, a.per_step) == ('list.txt', 540, 'owned.txt', 8)
    for bad in ([], ['c'], ['c', 'many']):
        with pytest.raises(SystemExit):
            complete_cube.parse_args(bad)
