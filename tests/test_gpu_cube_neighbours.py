"""The cube index and the exact k-nearest-cube search on the GPU, by direct calls
(cc_cube_index_put, cc_cube_neighbours): every row against the CPU oracle (tests/cube_sim_ref.py over
oracle/similarity_ref.py) and against the batched card path on the same matrix, bit for bit on
uint32 views.  Outputs, workspace and index buffer are filled with junk, a guard word stands behind
every output, and every case runs twice with different junk.

The kernels' own edges, beside the shapes every case runs:
  corpus chunk (64, 128, default)   -> N in {63, 64, 65} (one chunk, exactly, one cube more), 300 and
                                       1029 (a partial last chunk), 2504 (40 chunks of 64)
  k against a chunk's population    -> k = 40 with a last chunk of 5 or 44 cubes, k = cap above every
                                       chunk of 64 or 128, k above N (the -1 / 0 tail)
  query tile 32 / 64 / 128 (by Q)   -> Q in {1, 7, 65, 130}
  K stage 32                        -> K in {5, 32, 33, 70} next to 64
  put tile 128 rows                 -> N = 300, 1029 (not multiples), puts of 100-row pieces"""
import ctypes as C

import numpy as np
import pytest

from tests import cube_sim_ref as R
from tests.cube_sim_ref import u32

pytestmark = pytest.mark.gpu

GUARD = 0x5EEDC0DE
JUNK_I, JUNK_F = -77777, np.float32(-123.25)
JUNKS = (0x7FC0BEEF, 0x0BADF00D)
ENTRY = b'cc_cube_neighbours'


def lib():
    from cubecobrarecommender_amd import _lib as L
    return L.lib()


def max_k():
    return int(lib().cc_cube_neighbours_max_k())


def junk_buffer(nbytes, junk):
    import torch
    buf = torch.full((int(nbytes) // 4 + 64,), junk if junk < 2**31 else junk - 2**32, device='cuda',
                     dtype=torch.int32)
    assert buf.data_ptr() % 256 == 0
    return buf


class Index:
    """A junk-filled index buffer of capacity cap for K-float embeddings, and its puts."""

    def __init__(self, cap, K, junk=JUNKS[0]):
        self.cap, self.K = cap, K
        self.buf = junk_buffer(lib().cc_cube_index_size(cap, K), junk)

    def put(self, e, n0=0):
        import torch
        from cubecobrarecommender_amd import _lib as L
        z = torch.from_numpy(np.ascontiguousarray(e, np.float32).reshape(-1, self.K)).cuda()
        rows = 0 if e.size == 0 else z.shape[0]
        if rows == 0:
            z = torch.zeros(1, self.K, device='cuda')
        rc = lib().cc_cube_index_put(L.ptr(self.buf), self.cap, self.K, n0, rows, L.ptr(z), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, lib().cc_last_error_string()
        return self

    def bits(self):
        return self.buf.cpu().numpy().copy()


def search(index, N, qid, k, zq=None, skip=None, chunk=0, junk=JUNKS[0], Q=None):
    """A direct cc_cube_neighbours call on junk-filled outputs and workspace with a guard word
    behind both outputs: (idx [Q, k], dist [Q, k]); the call succeeded and the guards are intact."""
    import torch
    from cubecobrarecommender_amd import _lib as L
    Q = Q if Q is not None else (len(qid) if qid is not None else len(zq))
    q_d = torch.from_numpy(np.asarray(qid, np.int32)).cuda() if qid is not None else None
    z_d = torch.from_numpy(np.ascontiguousarray(zq, np.float32)).cuda() if zq is not None else None
    s_d = torch.from_numpy(np.asarray(skip, np.int32)).cuda() if skip is not None else None
    ws = junk_buffer(lib().cc_cube_neighbours_ws_size(N, index.K, Q, k, chunk), junk)
    oi = torch.full((Q * k + 1,), JUNK_I, device='cuda', dtype=torch.int32)
    od = torch.full((Q * k + 1,), float(JUNK_F), device='cuda', dtype=torch.float32)
    oi[-1] = GUARD
    od[-1] = float(np.array([GUARD], np.uint32).view(np.float32)[0])
    rc = lib().cc_cube_neighbours(L.ptr(index.buf), index.cap, N, index.K, Q, L.ptr(q_d), L.ptr(z_d), L.ptr(s_d),
                                  k, chunk, L.ptr(ws), L.ptr(oi), L.ptr(od), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().cc_last_error_string()
    oi_h, od_h = oi.cpu().numpy(), od.cpu().numpy()
    assert oi_h[-1:].view(np.uint32)[0] == GUARD and od_h[-1:].view(np.uint32)[0] == GUARD
    return oi_h[:-1].reshape(Q, k), od_h[:-1].reshape(Q, k)


def search_twice(index, N, qid, k, **kw):
    """The call with each junk: the two results agree in every bit."""
    gi, gd = search(index, N, qid, k, junk=JUNKS[0], **kw)
    gi2, gd2 = search(index, N, qid, k, junk=JUNKS[1], **kw)
    assert np.array_equal(gi, gi2) and np.array_equal(u32(gd), u32(gd2))
    return gi, gd


class Case:
    """One embedding matrix as an index on the device, and the oracle's distances, each once."""

    def __init__(self, kind, N, K, seed, cap=None):
        self.N, self.K = N, K
        self.e, self.special = R.make_emb(kind, N, K, seed)
        self.index = Index(cap or N, K).put(self.e)
        self._d = {}

    def dists(self, q):
        """(distances of member q to all cubes, their stable order)."""
        if q not in self._d:
            d = R.member_dists(self.e, q)
            self._d[q] = (d, np.argsort(d, kind='stable'))
        return self._d[q]

    def expected(self, qid, k, skip=None):
        rows = [R.expected_row(self.dists(int(q))[0], k, -1 if skip is None else int(skip[r]),
                               order=self.dists(int(q))[1]) for r, q in enumerate(qid)]
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def assert_rows(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(u32(got[1]), u32(want[1])), what


def k_values(N):
    cap = max_k()
    return sorted({1, 40, cap, min(N, cap)})


def check_case(case, Qs, seed, chunks=(64, 128, 0)):
    for Q in Qs:
        qid = R.make_queries(case.N, case.special, Q, seed)
        assert len(qid) == Q
        for k in k_values(case.N):
            want = case.expected(qid, k)
            for chunk in chunks:
                assert_rows(search_twice(case.index, case.N, qid, k, chunk=chunk), want, (Q, k, chunk))


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('N', [1, 63, 64, 65, 300, 1029, 2504])
def test_against_the_oracle(N, kind):
    check_case(Case(kind, N, 64, seed=N + 7 * R.KINDS.index(kind)), (1, 7, 65, 130), seed=N)


@pytest.mark.parametrize('kind', ['relu', 'signed'])
@pytest.mark.parametrize('K', [5, 32, 33, 70, 192])
def test_other_embedding_widths(K, kind):
    check_case(Case(kind, 300, K, seed=K), (1, 7, 65, 130), seed=K)


def test_query_tile_edges():
    """One query more than a tile of 32 and of 128 (65 is above); 65 cubes: a second cube tile of one."""
    check_case(Case('dups', 65, 64, seed=65), (33, 129), seed=65)


def test_duplicates_in_different_chunks():
    """Equal distances on both sides of chunk boundaries: lower cube id first, whatever the chunk."""
    N, K = 300, 64
    case = Case('relu', N, K, seed=41)
    pairs = ((10, 70), (10, 299), (63, 64), (127, 128), (5, 200))       # every pair straddles 64-cube chunks
    for a, b in pairs:
        assert a // 64 != b // 64
        case.e[b] = case.e[a]
    case.index = Index(N, K).put(case.e)
    qid = np.array([10, 70, 299, 63, 64, 127, 128, 5, 200, 0], np.int32)
    for k in (3, 40, N):
        want = case.expected(qid, k)
        assert want[0][0, 0] == 10 and want[0][1, 0] == 10               # the tie at the top: lower id first
        assert u32(want[1][0, :3]).tolist() == u32(want[1][1, :3]).tolist()
        for chunk in (64, 128, 0):
            assert_rows(search_twice(case.index, N, qid, k, chunk=chunk), want, (k, chunk))


@pytest.mark.parametrize('chunk', [64, 128, 0])
def test_all_zero_embeddings_rank_in_cube_order(chunk):
    N, k = 2504, max_k()
    case = Case('allzero', N, 64, seed=1)
    gi, gd = search_twice(case.index, N, [0, 1000, 2503], k, chunk=chunk)
    assert np.array_equal(gi, np.tile(np.arange(k, dtype=np.int32), (3, 1)))
    assert np.all(u32(gd) == 0x80000000)                                  # -0.0f
    assert_rows((gi, gd), case.expected([0, 1000, 2503], k), chunk)


def test_zero_rows_across_chunks():
    N = 300
    case = Case('relu', N, 64, seed=43)
    zero = [1, 2, 64, 130, 299]
    case.e[zero] = 0
    case.index = Index(N, 64).put(case.e)
    qid = np.array(zero + [0, 65], np.int32)
    for k in (5, 40, N):
        want = case.expected(qid, k)
        assert np.array_equal(want[0][0, :5], np.arange(5))               # a zero query: every distance -0
        for chunk in (64, 128, 0):
            assert_rows(search_twice(case.index, N, qid, k, chunk=chunk), want, (k, chunk))


@pytest.mark.parametrize('kind', R.KINDS)
def test_against_the_batched_card_path(kind):
    """Member queries, nothing skipped: the rows of cc_similar_cards_batch on the same matrix."""
    import torch
    from cubecobrarecommender_amd import _lib as L
    N, K, Q = 1029, 64, 130
    case = Case(kind, N, K, seed=51 + R.KINDS.index(kind))
    qid = R.make_queries(N, case.special, Q, 51)
    emb = torch.from_numpy(case.e).cuda()
    q_d = torch.from_numpy(qid).cuda()
    for k in (1, 40, max_k()):
        ws = junk_buffer(lib().cc_similar_batch_ws_size(N, K, Q, k), JUNKS[0])
        oi = torch.empty(Q, k, device='cuda', dtype=torch.int32)
        od = torch.empty(Q, k, device='cuda', dtype=torch.float32)
        L.call('cc_similar_cards_batch', L.ptr(emb), N, K, Q, L.ptr(q_d), k, L.ptr(ws), L.ptr(oi), L.ptr(od), None,
               L.stream_ptr())
        torch.cuda.synchronize()
        want = (oi.cpu().numpy(), od.cpu().numpy())
        for chunk in (64, 0):
            assert_rows(search_twice(case.index, N, qid, k, chunk=chunk), want, (k, chunk))


@pytest.mark.parametrize('kind', R.KINDS)
def test_member_against_fresh(kind):
    """qid = j and (qid = -1, zq[r] = emb[j]) give the same row; both kinds mixed in one call, with
    and without qid; a fresh embedding that is no member against the oracle."""
    N, K, k = 300, 64, 40
    case = Case(kind, N, K, seed=61 + R.KINDS.index(kind))
    ids = R.make_queries(N, case.special, 40, 61)
    rng = np.random.default_rng(62)
    zq = rng.standard_normal((len(ids), K)).astype(np.float32)            # junk where the row is a member
    qid = ids.copy()
    fresh = np.arange(len(ids)) % 2 == 1
    qid[fresh] = -1 - (np.arange(len(ids))[fresh] % 3) * 1000             # any negative id
    zq[fresh] = case.e[ids[fresh]]
    outside = case.e[7] * np.float32(0.5) + rng.standard_normal(K).astype(np.float32)
    want = case.expected(ids, k)
    for chunk in (64, 0):
        assert_rows(search_twice(case.index, N, ids, k, chunk=chunk), want, chunk)
        assert_rows(search_twice(case.index, N, qid, k, zq=zq, chunk=chunk), want, chunk)
        assert_rows(search_twice(case.index, N, None, k, zq=case.e[ids], chunk=chunk), want, chunk)
        gi, gd = search_twice(case.index, N, [-1, 7], k, zq=np.stack([outside, outside]), chunk=chunk)
        assert_rows((gi[:1], gd[:1]), [a[None] for a in R.expected_row(R.fresh_dists(case.e, outside), k)], chunk)
        assert_rows((gi[1:], gd[1:]), case.expected([7], k), chunk)


def test_skip():
    N, K = 300, 64
    case = Case('dups', N, K, seed=71)
    qid = R.make_queries(N, case.special, 30, 71)
    for k in (1, 40, 299, 300):
        for chunk in (64, 0):
            # the query itself: removes exactly that id and shifts the rest
            got = search_twice(case.index, N, qid, k, skip=qid, chunk=chunk)
            assert_rows(got, case.expected(qid, k, skip=qid), (k, chunk))
            assert not np.any(got[0] == qid[:, None])
            # outside [0, N): removes nothing
            for out in (-1, N, 2**31 - 1, -2**31):
                got = search_twice(case.index, N, qid, k, skip=np.full(len(qid), out), chunk=chunk)
                assert_rows(got, case.expected(qid, k), (k, chunk, out))
            # any other cube
            other = (qid + 101) % N
            assert_rows(search_twice(case.index, N, qid, k, skip=other, chunk=chunk),
                        case.expected(qid, k, skip=other), (k, chunk))
    # a skip in a chunk of exactly k cubes leaves k - 1 from it
    case64 = Case('relu', 128, K, seed=72)
    qid, skip = np.array([3, 100, 64], np.int32), np.array([3, 5, 127], np.int32)
    got = search_twice(case64.index, 128, qid, 64, skip=skip, chunk=64)
    assert_rows(got, case64.expected(qid, 64, skip=skip), 'k = chunk')
    one = Case('relu', 64, K, seed=73)
    got = search_twice(one.index, 64, [9], 64, skip=[9], chunk=64)
    assert_rows(got, one.expected([9], 64, skip=[9]), 'one chunk')
    assert got[0][0, 63] == -1 and u32(got[1])[0, 63] == 0 and np.all(got[0][0, :63] >= 0)
    # one cube, skipped: nothing is left
    single = Case('relu', 1, K, seed=74)
    gi, gd = search_twice(single.index, 1, [0, 0], 3, skip=[0, -1])
    assert np.all(gi[0] == -1) and np.all(u32(gd[0]) == 0)
    assert gi[1].tolist() == [0, -1, -1] and np.all(u32(gd[1, 1:]) == 0)


def test_invalid_queries_on_the_device():
    N, K, k = 300, 64, 12
    case = Case('relu', N, K, seed=81)
    qid = np.array([5, N, 299, 2**31 - 1, 5, -1, -2**31, 0], np.int64).astype(np.int32)
    valid = np.array([0 <= q < N for q in qid.tolist()])
    want = case.expected(qid[valid], k)
    for chunk in (64, 0):
        gi, gd = search_twice(case.index, N, qid, k, chunk=chunk)            # zq == NULL: the negative ids too
        assert_rows((gi[valid], gd[valid]), want, chunk)
        assert np.all(gi[~valid] == -1) and np.all(u32(gd[~valid]) == 0)
    # with zq the negative ids are fresh queries, the ids at or above N still nothing
    zq = np.tile(case.e[17], (len(qid), 1))
    gi, gd = search_twice(case.index, N, qid, k, zq=zq)
    assert_rows((gi[valid], gd[valid]), want, 'zq')
    fresh = qid < 0
    w17 = case.expected([17], k)
    for r in np.flatnonzero(fresh):
        assert_rows((gi[r:r + 1], gd[r:r + 1]), w17, r)
    rest = ~valid & ~fresh
    assert rest.sum() == 2 and np.all(gi[rest] == -1) and np.all(u32(gd[rest]) == 0)
    # no ids and no embeddings: no row is a query
    gi, gd = search_twice(case.index, N, None, k, Q=3)
    assert np.all(gi == -1) and np.all(u32(gd) == 0)


def test_piecewise_build():
    N, K, cap, k = 300, 64, 420, 40
    case = Case('dups', N, K, seed=91)
    whole = Index(cap, K, JUNKS[0]).put(case.e)
    pieces = Index(cap, K, JUNKS[1])
    for n0 in (200, 100, 0):                                              # descending, 100 rows each
        pieces.put(case.e[n0:n0 + 100], n0)
    pieces.put(case.e[:0], 50)                                            # rows == 0: nothing
    odd = Index(cap, K, JUNKS[1])
    for n0, n1 in ((130, 300), (0, 1), (1, 129), (129, 130)):             # pieces that split the put tile
        odd.put(case.e[n0:n1], n0)
    qid = R.make_queries(N, case.special, 30, 91)
    want = case.expected(qid, k)
    for index in (whole, pieces, odd):
        for chunk in (64, 0):
            assert_rows(search_twice(index, N, qid, k, chunk=chunk), want, chunk)
    # 37 more cubes: the old N still answers with the old bits, the new N as the oracle says
    more, _ = R.make_emb('relu', 37, K, seed=92)
    more[5] = case.e[10]                                                  # one of them ties with old cubes
    pieces.put(more, N)
    for chunk in (64, 0):
        assert_rows(search_twice(pieces, N, qid, k, chunk=chunk), want, chunk)
    grown = Case('relu', N + 37, K, seed=0, cap=cap)
    grown.e = np.concatenate([case.e, more])
    grown.index = pieces
    qid2 = np.concatenate([qid, np.array([N, N + 5, N + 36], np.int32)])
    want2 = grown.expected(qid2, k)
    for chunk in (64, 0):
        assert_rows(search_twice(pieces, N + 37, qid2, k, chunk=chunk), want2, chunk)


def test_guards_write_nothing():
    import torch
    from cubecobrarecommender_amd import _lib as L
    N, K, Q, k, cap = 300, 64, 4, 12, 320
    case = Case('relu', N, K, seed=13, cap=cap)
    index_before = case.index.bits()
    q_d = torch.tensor([1, 2, 3, 4], device='cuda', dtype=torch.int32)
    z_d = torch.zeros(Q, K, device='cuda')
    ws = torch.zeros(int(lib().cc_cube_neighbours_ws_size(N, K, Q, max_k(), 64)) // 4 + 64, device='cuda',
                     dtype=torch.int32)
    oi = torch.full((Q * (max_k() + 1),), JUNK_I, device='cuda', dtype=torch.int32)
    od = torch.full((Q * (max_k() + 1),), float(JUNK_F), device='cuda', dtype=torch.float32)

    def call(index=case.index.buf.data_ptr(), cap=cap, N=N, K=K, Q=Q, k=k, chunk=0, ws_ptr=ws.data_ptr(),
             out_idx=oi.data_ptr(), out_dist=od.data_ptr()):
        P = lambda a: None if a is None else C.c_void_p(a)               # noqa: E731
        rc = lib().cc_cube_neighbours(P(index), cap, N, K, Q, L.ptr(q_d), L.ptr(z_d), None, k, chunk, P(ws_ptr),
                                      P(out_idx), P(out_dist), L.stream_ptr())
        return rc, lib().cc_last_error_string()
    bad = [dict(index=None), dict(ws_ptr=None), dict(out_idx=None), dict(out_dist=None),
           dict(k=0), dict(k=-1), dict(k=max_k() + 1), dict(N=0), dict(N=-5), dict(N=cap + 1), dict(K=0), dict(K=-1),
           dict(chunk=-64), dict(chunk=1), dict(chunk=63), dict(chunk=100),
           dict(ws_ptr=ws.data_ptr() + 8), dict(ws_ptr=ws.data_ptr() + 128),
           dict(index=case.index.buf.data_ptr() + 16), dict(Q=-1)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and ENTRY in msg, kw
        rc, msg = call(**{**kw, 'Q': kw.get('Q', 0)})                     # with no rows, too
        assert rc == -1 and ENTRY in msg, kw
    assert call(Q=0)[0] == 0                                              # nothing launched
    # the put's own checks
    put = lib().cc_cube_index_put
    z = torch.zeros(8, K, device='cuda')
    for args in ((None, cap, K, 0, 8, L.ptr(z)), (L.ptr(case.index.buf), cap, K, 0, 8, None),
                 (C.c_void_p(case.index.buf.data_ptr() + 16), cap, K, 0, 8, L.ptr(z)),
                 (L.ptr(case.index.buf), cap, K, cap - 7, 8, L.ptr(z)), (L.ptr(case.index.buf), cap, K, -1, 8, L.ptr(z)),
                 (L.ptr(case.index.buf), cap, K, 0, -1, L.ptr(z)), (L.ptr(case.index.buf), 0, K, 0, 0, L.ptr(z)),
                 (L.ptr(case.index.buf), cap, 0, 0, 8, L.ptr(z))):
        assert put(*args, L.stream_ptr()) == -1 and b'cc_cube_index_put' in lib().cc_last_error_string(), args
    assert put(L.ptr(case.index.buf), cap, K, 5, 0, L.ptr(z), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((oi == JUNK_I).all()) and bool((od == float(JUNK_F)).all()) and bool((ws == 0).all())
    assert np.array_equal(case.index.bits(), index_before)


def test_one_larger_shape_against_similar_many():
    import torch
    from cubecobrarecommender_amd.similarity import similar_many
    N, K = 20000, 64
    case = Case('dups', N, K, seed=31)
    case.e[[1, 2, N - 1]] = 0
    case.index = Index(N, K).put(case.e)
    emb = torch.from_numpy(case.e).cuda()
    qid = np.array([0, N - 1, 10, 11, N - 2, 3, 1, 12345, 777, 19999, 64, 1023, 1024, 4096, 16384, 10], np.int32)
    for k in (40, max_k()):
        si, sd = similar_many(emb, qid, k)
        want = (si.astype(np.int32), sd)
        for chunk in (0, 4096):
            assert_rows(search_twice(case.index, N, qid, k, chunk=chunk), want, (k, chunk))
