"""Batched card similarity on the GPU (cc_similar_cards_batch, similar_many, similarity_table):
every row against the CPU oracle (oracle/similarity_ref.py) and, bit for bit, against the
single-request path (cc_similar_cards / similar()), whatever batch it falls into.

The kernels' own edges, beside the shapes every case runs (V 1..2504, Q 1..130, K 64):
  query tile 32 / 64 / 128 (chosen by Q)  -> Q in {32, 33, 64, 128, 129} next to 65 and 130
  card tile 64                            -> V in {63, 64, 65}; 1029 = 16 * 64 + 5
  K stage 32                              -> K in {5, 32, 33, 70} next to 64
  select / sort workgroup stride 1024     -> V = 1029 and 2504 (not multiples), V = 63 (below)
  normalise tile 128 rows                 -> V = 300, 1029 (not multiples), 63 (below)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from oracle import similarity_ref

pytestmark = pytest.mark.gpu

GUARD = 0x5EEDC0DE
JUNK_I, JUNK_F = -77777, np.float32(-123.25)
KINDS = ('relu', 'signed', 'zero-rows', 'dups', 'allzero', 'tiny')


def make_emb(kind, V, K, seed):
    """Finite embeddings of one kind, and the rows worth asking about."""
    rng = np.random.default_rng(seed)
    e = np.maximum(rng.standard_normal((V, K)).astype(np.float32), 0)
    special = []
    if kind == 'signed':
        e = (rng.standard_normal((V, K)) * np.exp2(rng.uniform(-8, 8, size=(V, K)))).astype(np.float32)
    elif kind == 'zero-rows':
        special = sorted({z for z in (1, 2, V - 1) if 0 <= z < V})
        e[special] = 0
    elif kind == 'dups' and V > 12:
        for a, b in ((10, 11), (10, V - 2), (3, 4)):
            e[b] = e[a]
        special = [10, 11, V - 2, 3, 4]
    elif kind == 'allzero':
        e[:] = 0
    elif kind == 'tiny':
        row = min(5, V - 1)
        e[row] = np.float32(1e-8) * (1 + rng.random(K)).astype(np.float32)       # ss <= 4 K 1e-16 < 1e-12
        assert float((e[row].astype(np.float64) ** 2).sum()) < 1e-12
        special = [row]
    assert np.all(np.isfinite(e))
    return e, special


def make_queries(V, special, Q, seed):
    """Q ids: 0 and V - 1, the special rows, the same id twice, then random ones."""
    rng = np.random.default_rng(seed + 1)
    head = [0, V - 1] + list(special) + [V // 2, V // 2]
    q = np.array(head + rng.integers(0, V, size=max(0, Q)).tolist(), np.int32)
    return q


def n_values(V, cap):
    return sorted({min(n, V) for n in (1, 40, cap, cap + 1, V)})


class Case:
    """One embedding on the device with its references, each computed once."""

    def __init__(self, kind, V, K, seed):
        import torch
        self.V, self.K = V, K
        self.e, self.special = make_emb(kind, V, K, seed)
        self.emb = torch.from_numpy(self.e).cuda()
        self._oracle, self._single, self._similar = {}, {}, {}

    def oracle(self, q):
        """(stable order, distances) of the CPU oracle for query q."""
        if q not in self._oracle:
            d = similarity_ref.cosine_dists(self.e, q)
            self._oracle[q] = (np.argsort(d, kind='stable'), d)
        return self._oracle[q]

    def single_dist_all(self, q):
        """cc_similar_cards' dist_all for query q (a direct call)."""
        import torch
        from cubecobrarecommender_amd import _lib as L
        if q not in self._single:
            V = self.V
            ws = torch.empty(int(L.lib().cc_similar_ws_size(V)) // 8 + 1, device='cuda', dtype=torch.int64)
            oi = torch.empty(1, device='cuda', dtype=torch.int32)
            od = torch.empty(1, device='cuda', dtype=torch.float32)
            da = torch.empty(V, device='cuda', dtype=torch.float32)
            L.call('cc_similar_cards', L.ptr(self.emb), V, self.K, int(q), 1, L.ptr(oi), L.ptr(od), L.ptr(da),
                   L.ptr(ws), L.stream_ptr())
            torch.cuda.synchronize()
            self._single[q] = da.cpu().numpy()
        return self._single[q]

    def similar(self, q, N):
        from cubecobrarecommender_amd.similarity import similar
        if (q, N) not in self._similar:
            self._similar[(q, N)] = similar(self.emb, q, N)
        return self._similar[(q, N)]


def batch_call(emb, V, K, queries, N, want_all, junk):
    """A direct cc_similar_cards_batch call on junk-filled outputs and workspace with a guard word
    behind every output: (rc, idx [Q, N], dist [Q, N], dist_all [Q, V] or None, guards intact)."""
    import torch
    from cubecobrarecommender_amd import _lib as L
    lib = L.lib()
    Q = len(queries)
    q_d = torch.from_numpy(np.asarray(queries, np.int32)).cuda()
    ws_bytes = int(lib.cc_similar_batch_ws_size(V, K, Q, N))
    ws = torch.full((ws_bytes // 4,), junk, device='cuda', dtype=torch.int32)
    assert ws.data_ptr() % 256 == 0
    oi = torch.full((Q * N + 1,), JUNK_I, device='cuda', dtype=torch.int32)
    od = torch.full((Q * N + 1,), float(JUNK_F), device='cuda', dtype=torch.float32)
    da = torch.full((Q * V + 1,), float(JUNK_F), device='cuda', dtype=torch.float32) if want_all else None
    guard_f = float(np.array([GUARD], np.uint32).view(np.float32)[0])     # the same bits as a float
    oi[-1] = GUARD
    od[-1] = guard_f
    if want_all:
        da[-1] = guard_f
    rc = lib.cc_similar_cards_batch(L.ptr(emb), V, K, Q, L.ptr(q_d), N, L.ptr(ws), L.ptr(oi), L.ptr(od),
                                    L.ptr(da), L.stream_ptr())
    torch.cuda.synchronize()
    oi_h, od_h = oi.cpu().numpy(), od.cpu().numpy()
    da_h = da.cpu().numpy() if want_all else None
    intact = (oi_h[-1:].view(np.uint32)[0] == GUARD and od_h[-1:].view(np.uint32)[0] == GUARD
              and (da_h is None or da_h[-1:].view(np.uint32)[0] == GUARD))
    return (rc, oi_h[:-1].reshape(Q, N), od_h[:-1].reshape(Q, N),
            None if da_h is None else da_h[:-1].reshape(Q, V), intact)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_case(case, Qs, seed):
    from cubecobrarecommender_amd import _lib as L
    from cubecobrarecommender_amd.similarity import SIM_NMAX
    V, K = case.V, case.K
    cap = int(L.lib().cc_similar_batch_max_n())
    for Q in Qs:
        queries = make_queries(V, case.special, Q, seed)[:Q]
        assert len(queries) == Q
        for N in n_values(V, cap):
            rc, idx, dist, dall, intact = batch_call(case.emb, V, K, queries, N, True, 0x7FC0BEEF)
            assert rc == 0 and intact, (Q, N)
            rc2, idx2, dist2, _, intact2 = batch_call(case.emb, V, K, queries, N, False, 0x0BADF00D)
            assert rc2 == 0 and intact2, (Q, N)
            assert np.array_equal(idx, idx2) and np.array_equal(u32(dist), u32(dist2)), (Q, N)
            for r, q in enumerate(queries.tolist()):
                order, d = case.oracle(q)
                assert np.array_equal(idx[r], order[:N]), (Q, N, r, q)
                assert np.array_equal(u32(dist[r]) & 0x7FFFFFFF, u32(d[order[:N]]) & 0x7FFFFFFF), (Q, N, r, q)
                assert np.array_equal(u32(dall[r]), u32(case.single_dist_all(q))), (Q, N, r, q)
                if N <= SIM_NMAX:
                    si, sd = case.similar(q, N)
                    assert np.array_equal(idx[r], si), (Q, N, r, q)
                    assert np.array_equal(u32(dist[r]), u32(sd)), (Q, N, r, q)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('V', [1, 63, 300, 1029, 2504])
def test_direct_calls_against_the_oracle_and_the_single_path(V, kind):
    check_case(Case(kind, V, 64, seed=V + 7 * KINDS.index(kind)), (1, 7, 65, 130), seed=V)


@pytest.mark.parametrize('kind', ['relu', 'signed'])
@pytest.mark.parametrize('K', [5, 32, 33, 70, 192])
def test_direct_calls_other_embedding_widths(K, kind):
    check_case(Case(kind, 300, K, seed=K), (1, 7, 65, 130), seed=K)


@pytest.mark.parametrize('V', [64, 65])
def test_direct_calls_at_the_tile_edges(V):
    check_case(Case('dups', V, 64, seed=V), (32, 33, 64, 128, 129), seed=V)


def test_all_zero_embeddings_rank_in_card_order():
    case = Case('allzero', 2504, 64, seed=1)
    rc, idx, dist, _, intact = batch_call(case.emb, 2504, 64, [0, 1000, 2503], 2504, False, 0x0BADF00D)
    assert rc == 0 and intact
    assert np.array_equal(idx, np.tile(np.arange(2504, dtype=np.int32), (3, 1)))
    assert np.all(u32(dist) == 0x80000000)                      # -0.0f, as the single path returns


def test_invalid_query_ids_on_the_device():
    V, K, N = 300, 64, 12
    case = Case('relu', V, K, seed=11)
    queries = [5, -1, 299, V, 5, 2**31 - 1, -2**31]
    rc, idx, dist, dall, intact = batch_call(case.emb, V, K, queries, N, True, 0x7FC0BEEF)
    assert rc == 0 and intact
    for r, q in enumerate(queries):
        if 0 <= q < V:
            si, sd = case.similar(q, N)
            assert np.array_equal(idx[r], si) and np.array_equal(u32(dist[r]), u32(sd))
            assert np.array_equal(u32(dall[r]), u32(case.single_dist_all(q)))
        else:
            assert np.all(idx[r] == -1) and np.all(u32(dist[r]) == 0), (r, q)
            assert np.all(u32(dall[r]) == 0), (r, q)
    from cubecobrarecommender_amd import _lib as L
    cap = int(L.lib().cc_similar_batch_max_n())
    assert cap < 2504                                           # the sort path, too
    big = Case('relu', 2504, K, seed=12)
    queries = [-1, 7, 2504]
    rc, idx, dist, _, intact = batch_call(big.emb, 2504, K, queries, cap + 1, False, 0x0BADF00D)
    assert rc == 0 and intact
    assert np.all(idx[[0, 2]] == -1) and np.all(u32(dist[[0, 2]]) == 0)
    si, sd = big.similar(7, cap + 1)
    assert np.array_equal(idx[1], si) and np.array_equal(u32(dist[1]), u32(sd))


def test_guards_write_nothing():
    import torch
    from cubecobrarecommender_amd import _lib as L
    lib = L.lib()
    V, K, Q, N = 300, 64, 4, 12
    case = Case('relu', V, K, seed=13)
    q_d = torch.tensor([1, 2, 3, 4], device='cuda', dtype=torch.int32)
    ws = torch.zeros(int(lib.cc_similar_batch_ws_size(V, K, Q, V)) // 4 + 64, device='cuda', dtype=torch.int32)
    oi = torch.full((Q * (V + 1),), JUNK_I, device='cuda', dtype=torch.int32)
    od = torch.full((Q * (V + 1),), float(JUNK_F), device='cuda', dtype=torch.float32)

    def call(Q=Q, N=N, ws_ptr=None, out_idx=oi):
        ws_p = L.ptr(ws) if ws_ptr is None else C.c_void_p(ws_ptr)
        rc = lib.cc_similar_cards_batch(L.ptr(case.emb), V, K, Q, L.ptr(q_d), N, ws_p, L.ptr(out_idx), L.ptr(od),
                                        None, L.stream_ptr())
        return rc, lib.cc_last_error_string()
    for kw in (dict(ws_ptr=ws.data_ptr() + 8), dict(out_idx=None), dict(N=0), dict(N=V + 1), dict(Q=-1)):
        rc, msg = call(**kw)
        assert rc == -1 and b'cc_similar_cards_batch' in msg, kw
    torch.cuda.synchronize()
    assert bool((oi == JUNK_I).all()) and bool((od == float(JUNK_F)).all()) and bool((ws == 0).all())


def test_similar_many_does_not_depend_on_the_batching():
    from cubecobrarecommender_amd.similarity import similar_many
    V, Q, N = 1029, 130, 40
    case = Case('dups', V, 64, seed=21)
    queries = make_queries(V, case.special, Q, 21)[:Q]
    base_i, base_d = similar_many(case.emb, queries, N)
    assert base_i.shape == (Q, N) and base_i.dtype == np.int64 and base_d.dtype == np.float32
    for r in (0, 1, 5, Q - 1):
        si, sd = case.similar(int(queries[r]), N)
        assert np.array_equal(base_i[r], si) and np.array_equal(u32(base_d[r]), u32(sd))
    for rows in (1, 3, 512):
        gi, gd = similar_many(case.emb, queries, N, rows_per_launch=rows)
        assert gi.tobytes() == base_i.tobytes() and gd.tobytes() == base_d.tobytes(), rows
        ri, rd = similar_many(case.emb, queries[::-1].copy(), N, rows_per_launch=rows)
        assert ri[::-1].tobytes() == base_i.tobytes() and rd[::-1].tobytes() == base_d.tobytes(), rows
    gi, gd = similar_many(case.emb, queries[:3], V + 9)          # n = min(N, V): every card, sorted
    assert gi.shape == (3, V) and np.array_equal(gi[0], case.oracle(int(queries[0]))[0])


def test_full_size_against_the_single_path():
    from cubecobrarecommender_amd import _lib as L
    from cubecobrarecommender_amd.similarity import SIM_NMAX, similar, similar_many
    V = 20884
    cap = int(L.lib().cc_similar_batch_max_n())
    assert cap + 1 <= SIM_NMAX
    case = Case('dups', V, 64, seed=31)
    case.e[[1, 2, V - 1]] = 0
    import torch
    case.emb = torch.from_numpy(case.e).cuda()
    queries = np.array([0, V - 1, 10, 11, V - 2, 3, 1, 12345, 777, 20000, 64, 1023, 1024, 4096, 19999, 10], np.int32)
    for N in (40, cap + 1):
        gi, gd = similar_many(case.emb, queries, N)
        for r, q in enumerate(queries.tolist()):
            si, sd = similar(case.emb, q, N)
            assert np.array_equal(gi[r], si), (N, r, q)
            assert np.array_equal(u32(gd[r]), u32(sd)), (N, r, q)


def test_similarity_table_and_cli(tmp_path):
    from cubecobrarecommender_amd.model import CC_Recommender, load_model
    from cubecobrarecommender_amd.similarity import card_embeddings, similar, similar_cards, similar_cards_many, \
        similarity_table
    V, d, N = 300, 64, 12
    model = CC_Recommender(V, d=d, dtype='bf16', seed=3)
    dest = str(tmp_path / 'ml_files' / 'high_req')
    model.save(dest, save_format='tf')
    m2 = load_model(dest)
    emb = card_embeddings(m2)
    want = [similar(emb, j, N) for j in range(V)]
    want_i, want_d = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    for source in (emb, m2):
        ti, td = similarity_table(source, N, rows_per_launch=128)
        assert ti.dtype == np.int32 and ti.shape == (V, N) and td.dtype == np.float32
        assert np.array_equal(ti, want_i) and np.array_equal(u32(td), u32(want_d))
    names = {i: f'card {i}' for i in range(V)}
    names[77] = 'lightning bolt'
    card_to_int = {v: k for k, v in names.items()}
    many = similar_cards_many(m2, ['lightning bolt', 'card 5', 'lightning bolt'], N, names, card_to_int)
    assert many[0] == many[2] == similar_cards(m2, 'lightning bolt', N, names, card_to_int)
    assert many[1] == similar_cards(m2, 'card 5', N, names, card_to_int)
    idmap = tmp_path / 'id_map.json'
    idmap.write_text(json.dumps({str(k): v for k, v in names.items()}))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from scripts import similarity_table as cli
    out = tmp_path / 'table.npz'
    lines = []
    cli.main([str(N), '--out', str(out), '--model-dir', dest, '--id-map', str(idmap)],
             print_fn=lambda *a: lines.append(' '.join(str(x) for x in a)))
    got = np.load(out)
    assert np.array_equal(got['indices'], want_i) and np.array_equal(u32(got['dists']), u32(want_d))
    assert got['names'].tolist() == [names[i] for i in range(V)]
    assert len(lines) == 1 and '300 cards x 12' in lines[0]
