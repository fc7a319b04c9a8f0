"""cc_cube_cluster and cc_cube_assign on the GPU by direct calls: every output against the CPU
reference (tests/cube_cluster_ref.py), bit for bit on uint32 views.  Index pads, workspace and
outputs are filled with junk, a guard word stands behind every output, and every case runs twice
with different junk (the two runs agree in every bit: the same call is repeatable).

The kernels' own edges:
  id block B and the 16 * RM row tile -> N in {1, 63, 64, 65, B - 1, B, B + 1, 1029, 2504}
  centroid tile 64                    -> k in {1, 2, 63, 64, 65, 130}, k == N included
  K stage 32, a lane per dimension    -> K in {5, 32, 33, 64, 70}
  max_iter                            -> 0, 1, 2, 50: n_iter, all of `changed`, and the invariant
                                         cc_cube_assign(members, returned centroids) == (label, dist)"""
import numpy as np
import pytest

from tests import cube_cluster_ref as R
from tests.cube_cluster_ref import u32
from tests.test_gpu_cube_neighbours import GUARD, JUNKS, Index, junk_buffer, lib

pytestmark = pytest.mark.gpu

JUNK_I, JUNK_F = -77777, np.float32(-123.25)
GUARD_F = float(np.array([GUARD], np.uint32).view(np.float32)[0])


def guarded(n, dtype, fill):
    import torch
    t = torch.full((n + 1,), fill, device='cuda', dtype=dtype)
    t[-1] = GUARD if dtype == torch.int32 else GUARD_F
    return t


def unguarded(t):
    h = t.cpu().numpy()
    assert h[-1:].view(np.uint32)[0] == GUARD
    return h[:-1]


def run_cluster(index, N, k, init, max_iter, junk=JUNKS[0]):
    """A direct cc_cube_cluster call: dict of the outputs; the call succeeded, the guards hold."""
    import torch
    from cubecobrarecommender_amd import _lib as L
    K = index.K
    ids = torch.from_numpy(np.asarray(init, np.int32)).cuda()
    ws = junk_buffer(lib().cc_cube_cluster_ws_size(N, K, k, 0), junk)
    lab, dist = guarded(N, torch.int32, JUNK_I), guarded(N, torch.float32, float(JUNK_F))
    cent, sizes = guarded(k * K, torch.float32, float(JUNK_F)), guarded(k, torch.int32, JUNK_I)
    changed, n_iter = guarded(max_iter + 1, torch.int32, JUNK_I), guarded(1, torch.int32, JUNK_I)
    rc = lib().cc_cube_cluster(L.ptr(index.buf), index.cap, N, K, k, L.ptr(ids), max_iter, L.ptr(ws), L.ptr(lab),
                               L.ptr(dist), L.ptr(cent), L.ptr(sizes), L.ptr(changed), L.ptr(n_iter), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().cc_last_error_string()
    return dict(label=unguarded(lab), dist=unguarded(dist), centroids=unguarded(cent).reshape(k, K),
                sizes=unguarded(sizes), changed=unguarded(changed), n_iter=int(unguarded(n_iter)[0]))


def run_assign(index, N, centroids, qid=None, zq=None, Q=None, junk=JUNKS[0]):
    """A direct cc_cube_assign call: (label [Q], dist [Q])."""
    import torch
    from cubecobrarecommender_amd import _lib as L
    K, k = index.K, len(centroids)
    Q = Q if Q is not None else (len(qid) if qid is not None else len(zq))
    c_d = torch.from_numpy(np.ascontiguousarray(centroids, np.float32)).cuda()
    q_d = torch.from_numpy(np.asarray(qid, np.int32)).cuda() if qid is not None else None
    z_d = torch.from_numpy(np.ascontiguousarray(zq, np.float32)).cuda() if zq is not None else None
    ws = junk_buffer(lib().cc_cube_cluster_ws_size(0, K, k, Q), junk)
    lab, dist = guarded(Q, torch.int32, JUNK_I), guarded(Q, torch.float32, float(JUNK_F))
    rc = lib().cc_cube_assign(L.ptr(index.buf), index.cap, N, K, k, L.ptr(c_d), Q, L.ptr(q_d), L.ptr(z_d), L.ptr(ws),
                              L.ptr(lab), L.ptr(dist), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().cc_last_error_string()
    return unguarded(lab), unguarded(dist)


def same(got, want):
    return all(np.array_equal(u32(np.asarray(got[f])), u32(np.asarray(want[f])))
               for f in ('label', 'dist', 'centroids', 'sizes', 'changed')) and got['n_iter'] == want['n_iter']


def field_diffs(got, want):
    return {f: int((u32(np.asarray(got[f])) != u32(np.asarray(want[f]))).sum())
            for f in ('label', 'dist', 'centroids', 'sizes', 'changed')}, got['n_iter'], want['n_iter']


class Case:
    """One embedding matrix as a junk-filled index on the device (capacity above N where asked) and
    its reference rows."""

    def __init__(self, kind, N, K, seed, cap=None):
        self.N, self.K = N, K
        self.e, self.special = R.make_emb(kind, N, K, seed)
        self.n = R.normalise(self.e)
        self.index = Index(cap or N, K).put(self.e)

    def check(self, k, init, max_iter, assign_back=True):
        """Both junks give the reference's bits; the returned labels are the assign of the returned
        centroids."""
        want = R.cluster(self.n, init, max_iter)
        for junk in JUNKS:
            got = run_cluster(self.index, self.N, k, init, max_iter, junk=junk)
            assert same(got, want), (k, max_iter, field_diffs(got, want))
        if assign_back:
            lab, dist = run_assign(self.index, self.N, got['centroids'], qid=np.arange(self.N), junk=JUNKS[1])
            assert np.array_equal(lab, got['label']) and np.array_equal(u32(dist), u32(got['dist']))
        return want


def ks_of(N):
    return sorted({k for k in (1, 2, 63, 64, 65, 130, N) if k <= N and k <= 130})


def block():
    return int(lib().cc_cube_cluster_block())


def n_values():
    B = 256          # asserted against the library in test_block_is_the_librarys
    return [1, 63, 64, 65, B - 1, B, B + 1, 1029, 2504]


def test_block_is_the_librarys():
    assert block() == 256 and int(lib().cc_cube_cluster_max_k()) >= 1024


@pytest.mark.parametrize('N', n_values())
def test_sizes_against_the_reference(N):
    """Every N at every k it admits, relu rows, to convergence; the smallest and the largest k at
    every max_iter."""
    case = Case('relu', N, 64, seed=N)
    ks = ks_of(N)
    for k in ks:
        want = case.check(k, R.init_ids(N, k, seed=N + k), 50)
        assert want['converged'] and want['n_iter'] < 50
    for k in (ks[0], ks[-1]):
        for max_iter in (0, 1, 2):
            case.check(k, R.init_ids(N, k, seed=N + k), max_iter)


@pytest.mark.parametrize('kind', R.KINDS)
def test_kinds_against_the_reference(kind):
    N, K = 1029, 64
    case = Case(kind, N, K, seed=7 * R.KINDS.index(kind) + 3)
    for k in (2, 65, 130):
        init = R.init_ids(N, k, seed=k)
        if kind == 'dups':
            init[:2] = (10, 11)                       # equal rows: every distance to both is equal
        wants = {max_iter: case.check(k, init, max_iter) for max_iter in (0, 1, 50)}
        want = wants[50]
        assert want['converged'] and want['n_iter'] < 50
        if kind == 'dups':                            # the first assign leaves the second centroid empty,
            assert wants[0]['sizes'][1] == 0          # and the update then keeps its bits
            assert np.array_equal(u32(wants[1]['centroids'][1]), u32(case.n[11]))
        if kind == 'allzero':
            assert np.all(want['label'] == 0) and np.all(want['sizes'][1:] == 0) and want['sizes'][0] == N
            assert np.all(u32(want['dist']) == 0x80000000)        # -0.0f
        if kind == 'planted' and k == 130:
            assert (want['sizes'] == 0).any()


@pytest.mark.parametrize('kind', ['relu', 'signed'])
@pytest.mark.parametrize('K', [5, 32, 33, 70])
def test_other_embedding_widths(K, kind):
    N = 300
    case = Case(kind, N, K, seed=K)
    for k in (2, 65):
        for max_iter in (1, 50):
            case.check(k, R.init_ids(N, k, seed=K + k), max_iter)


def test_a_corpus_large_enough_for_several_centroid_tiles_per_workgroup():
    """Below about 2,048 row tiles a row tile's centroid tiles are spread over workgroups (every
    other case here); 140,000 cubes at k = 130 leave two of the three tiles to one workgroup.  K = 5
    keeps the reference short."""
    N, K, k = 140000, 5, 130
    case = Case('relu', N, K, seed=17)
    init = R.init_ids(N, k, seed=17)
    want = R.cluster(case.n, init, 1)
    got = run_cluster(case.index, N, k, init, 1)
    assert same(got, want), field_diffs(got, want)
    lab, dist = run_assign(case.index, N, got['centroids'], qid=np.arange(N), junk=JUNKS[1])
    assert np.array_equal(lab, got['label']) and np.array_equal(u32(dist), u32(got['dist']))


def test_capacity_above_n_reads_nothing_behind_n():
    """The rows behind N stay junk (NaN bits): any read of them would poison a distance."""
    N, K, cap = 300, 64, 420
    case = Case('relu', N, K, seed=5, cap=cap)
    for k in (3, 65):
        case.check(k, R.init_ids(N, k, seed=k), 50)
    part = Case('relu', N, K, seed=5, cap=cap)        # the same rows; a clustering of the first 257
    want = R.cluster(part.n[:257], R.init_ids(257, 5, seed=1), 50)
    got = run_cluster(part.index, 257, 5, R.init_ids(257, 5, seed=1), 50)
    assert same(got, want), field_diffs(got, want)


def test_duplicate_and_clamped_init_ids():
    N, K, k = 300, 64, 4
    case = Case('relu', N, K, seed=9)
    case.check(k, [7, 7, 7, 7], 50)                   # all start equal: cluster 0 takes every cube
    want = R.cluster(case.n, [0, N - 1, 5, N - 1], 3)
    got = run_cluster(case.index, N, k, [-5, N + 7, 5, 2**31 - 1], 3)     # clamped, never an index
    assert same(got, want), field_diffs(got, want)


def test_assign_member_fresh_and_invalid_rows():
    N, K, k = 300, 64, 65
    case = Case('dups', N, K, seed=21)
    rng = np.random.default_rng(22)
    cents = rng.standard_normal((k, K)).astype(np.float32)                # any rows: taken as they are
    cents[5] = cents[4]                                                   # equal distances: the lower id
    ids = np.array([0, N - 1, 10, 11, 3, 3] + rng.integers(0, N, 130).tolist(), np.int32)
    wl, wd = R.assign(case.n[ids], cents)
    assert not np.any(wl == 5)
    for junk in JUNKS:
        gl, gd = run_assign(case.index, N, cents, qid=ids, junk=junk)
        assert np.array_equal(gl, wl) and np.array_equal(u32(gd), u32(wd))
        gl, gd = run_assign(case.index, N, cents, zq=case.e[ids], junk=junk)       # fresh: the put's arithmetic
        assert np.array_equal(gl, wl) and np.array_equal(u32(gd), u32(wd))
    qid = np.array([5, N, -1, 2**31 - 1, 299, -2**31], np.int64).astype(np.int32)
    gl, gd = run_assign(case.index, N, cents, qid=qid)                    # zq == NULL: the negative ids too
    valid = np.array([0 <= q < N for q in qid.tolist()])
    wl, wd = R.assign(case.n[qid[valid]], cents)
    assert np.array_equal(gl[valid], wl) and np.array_equal(u32(gd[valid]), u32(wd))
    assert np.all(gl[~valid] == -1) and np.all(u32(gd[~valid]) == 0)
    zq = np.tile(case.e[17], (len(qid), 1))
    gl, gd = run_assign(case.index, N, cents, qid=qid, zq=zq)
    w17 = R.assign(case.n[17:18], cents)
    for r in np.flatnonzero(qid < 0):
        assert gl[r] == w17[0][0] and u32(gd[r:r + 1])[0] == u32(w17[1])[0]
    outside = (case.e[7] * np.float32(0.5) + rng.standard_normal(K).astype(np.float32))[None]
    gl, gd = run_assign(case.index, N, cents, zq=outside)
    wl, wd = R.assign(R.normalise(outside), cents)
    assert np.array_equal(gl, wl) and np.array_equal(u32(gd), u32(wd))


def test_bad_arguments_launch_nothing():
    import ctypes as C
    import torch
    from cubecobrarecommender_amd import _lib as L
    N, K, k, cap = 300, 64, 5, 320
    case = Case('relu', N, K, seed=13, cap=cap)
    before = case.index.bits()
    out = torch.full((4096,), JUNK_I, device='cuda', dtype=torch.int32)
    ws = torch.zeros(int(lib().cc_cube_cluster_ws_size(N, K, k, 8)) // 4 + 64, device='cuda', dtype=torch.int32)
    ids = torch.zeros(k, device='cuda', dtype=torch.int32)
    P = lambda a: None if a is None else C.c_void_p(a)                   # noqa: E731
    o = out.data_ptr()

    def call(index=case.index.buf.data_ptr(), cap=cap, N=N, K=K, k=k, init=ids.data_ptr(), max_iter=3,
             ws_ptr=ws.data_ptr(), label=o):
        rc = lib().cc_cube_cluster(P(index), cap, N, K, k, P(init), max_iter, P(ws_ptr), P(label), P(o + 4096),
                                   P(o + 8192), P(o + 12288), P(o + 14000), P(o + 16000), L.stream_ptr())
        return rc, lib().cc_last_error_string()
    for kw in (dict(index=None), dict(init=None), dict(ws_ptr=None), dict(label=None), dict(k=0), dict(k=-1),
               dict(k=N + 1), dict(k=int(lib().cc_cube_cluster_max_k()) + 1, N=cap), dict(max_iter=-1), dict(N=-1),
               dict(N=cap + 1), dict(K=0), dict(cap=0), dict(ws_ptr=ws.data_ptr() + 8),
               dict(index=case.index.buf.data_ptr() + 16)):
        rc, msg = call(**kw)
        assert rc == -1 and b'cc_cube_cluster' in msg, kw
    assert call(N=0)[0] == 0

    def assign(index=case.index.buf.data_ptr(), N=N, K=K, k=k, cents=o + 8192, Q=8, ws_ptr=ws.data_ptr(), label=o):
        rc = lib().cc_cube_assign(P(index), cap, N, K, k, P(cents), Q, P(ids.data_ptr()), None, P(ws_ptr), P(label),
                                  P(o + 4096), L.stream_ptr())
        return rc, lib().cc_last_error_string()
    for kw in (dict(index=None), dict(cents=None), dict(ws_ptr=None), dict(label=None), dict(k=0),
               dict(k=int(lib().cc_cube_cluster_max_k()) + 1), dict(N=-1), dict(N=cap + 1), dict(K=0), dict(Q=-1),
               dict(ws_ptr=ws.data_ptr() + 128)):
        rc, msg = assign(**kw)
        assert rc == -1 and b'cc_cube_assign' in msg, kw
    assert assign(Q=0)[0] == 0
    torch.cuda.synchronize()
    assert bool((out == JUNK_I).all()) and bool((ws == 0).all())
    assert np.array_equal(case.index.bits(), before)
