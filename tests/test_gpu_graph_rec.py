"""cc_graph_rec_f64 / cc_graph_rec_target_ranks_f64 / GraphRecommender on the device against the
numpy statement of the pinned definition (tests/graph_rec_ref.py).  Every comparison is exact:
f64 bit patterns and integers, np.array_equal, no tolerance anywhere."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.adjacency import adjacency_device, upload_lists
from cubecobrarecommender_amd.evaluate import evaluate_holdout, holdout_split, metrics_from_ranks
from cubecobrarecommender_amd.graphrec import GraphRecommender
from cubecobrarecommender_amd.recommender import pack_cubes
from oracle import adjacency_ref
from tests import graph_rec_ref as G

pytestmark = pytest.mark.gpu

# one lane; below one wave; odd, a tile of 256 and part of the next; odd, past the 256-, 512- and
# 1024-column tile edges; even, and a cube of V - 1 cards needs three LDS chunks of 1024 ids
SHAPES = [1, 63, 300, 1029, 2504]
KINDS = ['counts', 'wild', 'negzero', 'equal', 'sentinel']
WIDE = 16          # cubes per call from which a lane owns two columns
GUARD = 16
_matrices, _scores = {}, {}


def sparse_lists(rng, V, C=30):
    pop = 1.0 / (1.0 + rng.permutation(V))
    pop /= pop.sum()
    return [np.sort(rng.choice(V, min(V, int(rng.integers(1, 25))), replace=False, p=pop)) for _ in range(C)]


def matrix_of(V, kind):
    """The test matrices [V][V] f64, built once:
      counts    oracle.adjacency_ref of sparse synthetic cubes (counts / diagonal): most scores tie
      wild      normal times 2^U(-40, 40), negatives included: another summation order changes bits
      negzero   entries from {-0.0, +0.0, 1, -1}: zero sums of either sign's making, long ties
      equal     every entry 0.25: every row ties
      sentinel  wild with the diagonal at 1e30: it must show up in no score"""
    if (V, kind) not in _matrices:
        rng = np.random.default_rng(1000 + V)
        if kind == 'counts':
            M = adjacency_ref.adjacency_from_lists(sparse_lists(rng, V), V)
        elif kind in ('wild', 'sentinel'):
            M = rng.normal(size=(V, V)) * np.exp2(rng.uniform(-40, 40, size=(V, V)))
            if kind == 'sentinel':
                np.fill_diagonal(M, 1e30)
        elif kind == 'negzero':
            M = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), size=(V, V))
        else:
            M = np.full((V, V), 0.25)
        _matrices[(V, kind)] = np.ascontiguousarray(M, np.float64)
    return _matrices[(V, kind)]


def edge_cubes(V, rows=20):
    """n in {0, 1, 2, 45, V - 1, V} (clipped to V), cards 0 and V - 1, cards on both sides of every
    wave and tile edge of the scoring kernel (64, 128, 256, 512, ...), then random cubes: `rows`
    cubes, the first seven the edge cases."""
    rng = np.random.default_rng(V)
    every = np.arange(V)
    edges = np.array([c for c in (0, 63, 64, 127, 128, 255, 256, 257, 511, 512, 767, 768, 1023, 1024, V - 1) if c < V])
    mid = 256 if V > 257 else V // 2
    extra = rng.choice(np.setdiff1d(every, edges), max(0, min(V, 45) - len(np.unique(edges))), replace=False)
    cubes = [np.zeros(0, np.int64), np.array([0]), np.array([V - 1]), np.unique([0, V - 1]),
             np.unique(np.concatenate([edges, extra])), every[every != mid] if V > 1 else every, every]
    while len(cubes) < rows:
        cubes.append(rng.choice(V, int(rng.integers(1, min(V, 120) + 1)), replace=False))
    return [np.asarray(c, np.int64) for c in cubes]


def ref_scores(V, kind, tag, cubes):
    if (V, kind, tag) not in _scores:
        M = matrix_of(V, kind)
        _scores[(V, kind, tag)] = [G.scores(M, c) for c in cubes]
    return _scores[(V, kind, tag)]


def device_matrix(M, pad):
    """M on the device with a row pitch of V + pad -> (tensor [V, V + pad] holding junk in the pad, ld)."""
    V = M.shape[0]
    buf = torch.full((V, V + pad), 3e33, dtype=torch.float64, device='cuda')
    buf[:, :V] = torch.from_numpy(M).cuda()
    return buf, V + pad


def guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, device='cuda', dtype=dtype)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _direct(buf, ld, V, cubes, amount, want_scores=True, R=None, ws_shift=0, null=None):
    """cc_graph_rec_f64 itself: outputs and workspace pre-filled with junk, guard words behind."""
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    Rr, nnz, A = len(cubes), len(idx), max(amount, 1)
    rp = torch.from_numpy(row_ptr).cuda()
    ix = torch.from_numpy(idx if nnz else np.zeros(1, np.int32)).cuda()
    ws = torch.full((int(L.lib().cc_graph_rec_ws_size(V, Rr, max_n)) // 4 + 64,), -1, device='cuda', dtype=torch.int32)
    assert ws.data_ptr() % 256 == 0
    nadd, adds = guarded(Rr, torch.int32, 77), guarded(Rr * A, torch.int32, 77)
    addv, cutv = guarded(Rr * A, torch.float64, 7.0), guarded(nnz, torch.float64, 7.0)
    sc = guarded(Rr * V, torch.float64, 7.0) if want_scores else None
    rc = L.lib().cc_graph_rec_f64(
        L.ptr(buf), ld, V, Rr if R is None else R, L.ptr(rp), L.ptr(ix), max_n, amount,
        L.C.c_void_p(ws.data_ptr() + ws_shift), None if null == 'n_add' else L.ptr(nadd), L.ptr(adds), L.ptr(addv),
        L.ptr(cutv), L.ptr(sc), L.stream_ptr())
    torch.cuda.synchronize()
    out = dict(rc=rc, row_ptr=row_ptr, idx=idx, A=A)
    for name, t, n, fill in (('nadd', nadd, Rr, 77), ('adds', adds, Rr * A, 77), ('addv', addv, Rr * A, 7.0),
                             ('cutv', cutv, nnz, 7.0), ('scores', sc, Rr * V, 7.0)):
        if t is None:
            continue
        h = t.cpu().numpy()
        assert np.all(h[n:] == fill), f'guard words behind {name}'
        out[name] = h[:n]
    return out


def check_rows(out, V, cubes, want, amount):
    """Every output of a direct call against the reference, row by row."""
    A = out['A']
    adds, addv = out['adds'].reshape(len(cubes), A), out['addv'].reshape(len(cubes), A)
    for r, (cube, s) in enumerate(zip(cubes, want)):
        ea, ev = G.additions(s, cube, amount)
        k = min(max(amount, 1), V - len(cube))
        assert len(ea) == max(k, 0) and out['nadd'][r] == k, r
        assert np.array_equal(adds[r, :k], ea), r
        assert np.array_equal(bits(addv[r, :k]), bits(ev)), r
        assert np.all(adds[r, k:] == -1) and np.array_equal(bits(addv[r, k:]), bits(np.zeros(A - k))), r
        lo, hi = out['row_ptr'][r], out['row_ptr'][r + 1]
        assert np.array_equal(out['idx'][lo:hi], np.unique(cube))
        assert np.array_equal(bits(out['cutv'][lo:hi]), bits(s[np.unique(cube)])), r
        if 'scores' in out:
            assert np.array_equal(bits(out['scores'].reshape(len(cubes), V)[r]), bits(s)), r


@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('V', SHAPES)
def test_direct_call(V, pad):
    """All five matrices, the edge cubes, every amount, one column per lane (7 cubes) and two
    (20 cubes); pad 3 gives an odd pitch (8-byte loads) for even V and an even pitch with an odd
    V (16-byte loads and a last lone column) for odd V."""
    cap = int(L.lib().cc_graph_rec_max_amount())
    cubes = edge_cubes(V)
    assert sorted({len(c) for c in cubes[:7]}) == sorted({0, 1, min(2, V), min(45, V), max(V - 1, 1), V})
    for kind in KINDS:
        M = matrix_of(V, kind)
        buf, ld = device_matrix(M, pad)
        want = ref_scores(V, kind, 'edge', cubes)
        if kind == 'sentinel':
            assert all(np.all(np.abs(s) < 1e29) for s in want)
        if kind == 'counts' and V >= 300:
            assert all(len(np.unique(s)) < V // 4 for s in want[:3])               # most scores tie
        for amount in (0, 1, 100, cap):
            for rows in (len(cubes), 7):
                assert (rows >= WIDE) == (rows == len(cubes))
                out = _direct(buf, ld, V, cubes[:rows], amount, want_scores=(amount != 1))
                assert out['rc'] == 0
                check_rows(out, V, cubes[:rows], want[:rows], amount)


def test_zero_signs_and_full_ties():
    """-0.0 ranks as +0.0 and no score is -0.0; with every entry equal the additions are the
    missing cards from the highest index down and the cuts the cube from the lowest up."""
    V = 300
    cubes = edge_cubes(V)
    rec = GraphRecommender(matrix_of(V, 'negzero'))
    outs = rec.recommend_many(cubes, 100, want_scores=True)
    for o, s in zip(outs, ref_scores(V, 'negzero', 'edge', cubes)):
        assert not np.any(np.signbit(o['scores'][o['scores'] == 0.0]))
        assert np.array_equal(bits(o['scores']), bits(s))
    assert sum(int(np.count_nonzero(o['scores'] == 0.0)) for o in outs) > V
    rec = GraphRecommender(matrix_of(V, 'equal'))
    for cube, o in zip(cubes, rec.recommend_many(cubes, 100)):
        missing = np.setdiff1d(np.arange(V), cube)
        assert np.array_equal(o['additions'], missing[::-1][:100])
        assert np.array_equal(o['cuts'], np.unique(cube))
        assert np.all(o['add_vals'] == 0.25 * len(cube)) and np.all(o['cut_vals'] == 0.25 * max(len(cube) - 1, 0))


def same(a, b, keys=('additions', 'add_vals', 'cuts', 'cut_vals')):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


@pytest.mark.parametrize('pad', [0, 3])
def test_batching(pad):
    """A row's results are the same bits alone, in any batch and in any launch split (the split
    changes how many columns a lane owns and the load width), twice, and on a workspace full of
    0xFF."""
    V, kind = 1029, 'wild'
    M = matrix_of(V, kind)
    buf, ld = device_matrix(M, pad)
    rec = GraphRecommender(buf[:, :V])
    assert rec.ld == ld and rec.adj.data_ptr() == buf.data_ptr()        # used in place
    rng = np.random.default_rng(7)
    cubes = edge_cubes(V, rows=8) + [rng.choice(V, int(rng.integers(1, 400)), replace=True) for _ in range(122)]
    assert len(cubes) == 130
    want = ref_scores(V, kind, 'batch', cubes)
    base = rec.recommend_many(cubes, 100, want_scores=True, rows_per_launch=64)
    for r, (cube, s, o) in enumerate(zip(cubes, want, base)):
        ea, ev = G.additions(s, cube, 100)
        ec, ecv = G.cuts(s, cube)
        assert o['additions'].dtype == np.int32 and o['add_vals'].dtype == np.float64
        assert o['cuts'].dtype == np.int32 and o['cut_vals'].dtype == np.float64
        assert np.array_equal(o['additions'], ea) and np.array_equal(bits(o['add_vals']), bits(ev)), r
        assert np.array_equal(o['cuts'], ec) and np.array_equal(bits(o['cut_vals']), bits(ecv)), r
        assert np.array_equal(bits(o['scores']), bits(s)), r
    for split in (512, 64, 7):
        rec._ws.buf.fill_(-1)
        torch.cuda.synchronize()                                           # the fill ran on another stream
        again = rec.recommend_many(cubes, 100, rows_per_launch=split)          # without the scores
        assert len(again) == 130 and all(same(a, b) for a, b in zip(again, base)) and 'scores' not in again[0]
    for R in (1, 3, WIDE - 1, WIDE, WIDE + 1):
        part = rec.recommend_many(cubes[:R], 100, want_scores=True)
        assert all(same(a, b, ('additions', 'add_vals', 'cuts', 'cut_vals', 'scores')) for a, b in zip(part, base))
    for r in (0, 4, 6, 77, 129):
        assert same(rec.recommend(cubes[r], 100), base[r])


def ranks_direct(buf, ld, V, cubes, targets, cutoffs=(), want_hits=None, n_cut=None):
    """cc_graph_rec_target_ranks_f64 itself, outputs and workspace pre-filled with junk."""
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    tgt_ptr = np.zeros(len(cubes) + 1, np.int32)
    tgt_ptr[1:] = np.cumsum([len(t) for t in targets])
    tgt = np.concatenate([np.asarray(t, np.int64) for t in targets]).astype(np.int32)
    nt = len(tgt)
    want_hits = bool(len(cutoffs)) if want_hits is None else want_hits

    def dev_of(a):
        return torch.from_numpy(a if len(a) else np.zeros(1, np.int32)).cuda()
    rp, ix, tp, tg = dev_of(row_ptr), dev_of(idx), dev_of(tgt_ptr), dev_of(tgt)
    cut = torch.tensor(list(cutoffs) or [0], device='cuda', dtype=torch.int32)
    ws = torch.full((int(L.lib().cc_graph_rec_ws_size(V, len(cubes), max_n)) // 4 + 64,), -1, device='cuda',
                    dtype=torch.int32)
    ranks, vals = guarded(nt, torch.int32, 77), guarded(nt, torch.float64, 7.0)
    cutv = guarded(len(idx), torch.float64, 7.0)
    hits = torch.zeros(len(cutoffs) + 2 + GUARD, device='cuda', dtype=torch.int64) if want_hits else None
    rc = L.lib().cc_graph_rec_target_ranks_f64(
        L.ptr(buf), ld, V, len(cubes), L.ptr(rp), L.ptr(ix), max_n, L.ptr(tp), L.ptr(tg),
        L.ptr(cut) if len(cutoffs) else None, len(cutoffs) if n_cut is None else n_cut, L.ptr(ws), L.ptr(ranks),
        L.ptr(vals), L.ptr(hits), L.ptr(cutv), None, L.stream_ptr())
    torch.cuda.synchronize()
    r, v, c = ranks.cpu().numpy(), vals.cpu().numpy(), cutv.cpu().numpy()
    assert np.all(r[nt:] == 77) and np.all(v[nt:] == 7.0) and np.all(c[len(idx):] == 7.0)
    h = None
    if want_hits:
        h = hits.cpu().numpy()
        assert np.all(h[len(cutoffs) + 2:] == 0)
        h = h[:len(cutoffs) + 2]
    return dict(rc=rc, tgt_ptr=tgt_ptr, ranks=r[:nt], vals=v[:nt], hits=h, cutv=c[:len(idx)], row_ptr=row_ptr, idx=idx)


def target_rows(V):
    """(cubes, targets): no targets, every candidate in order and shuffled, duplicates, invalid
    ids (-1, V, huge, in the cube), a full cube, and rows past the 16 waves of a workgroup."""
    rng = np.random.default_rng(50 + V)
    every = np.arange(V)
    cubes, targets = [], []

    def row(cube, tgt):
        cubes.append(np.asarray(cube, np.int64))
        targets.append(np.asarray(tgt, np.int64))
    row([], [])
    row([], rng.permutation(V))
    c = rng.choice(V, 33, replace=False)
    row(c, [np.setdiff1d(every, c)[5]])
    c = rng.choice(V, 20, replace=False)
    row(c, np.setdiff1d(every, c))
    c = rng.choice(V, 15, replace=False)
    t = rng.choice(np.setdiff1d(every, c), 12, replace=False)
    row(c, rng.permutation(np.concatenate([t, t[:7], t[2:4]])))
    c = rng.choice(V, 25, replace=False)
    t = rng.choice(np.setdiff1d(every, c), 6, replace=False)
    row(c, [t[0], c[3], t[1], V, t[2], -1, t[3], 2 ** 31 - 1, t[4], t[5]])
    row(rng.permutation(V), [])
    while len(cubes) < 18:
        c = rng.choice(V, int(rng.integers(1, 40)), replace=False)
        row(c, rng.choice(np.setdiff1d(every, c), int(rng.integers(1, 20)), replace=False))
    return cubes, targets


@pytest.mark.parametrize('kind', ['counts', 'wild'])
@pytest.mark.parametrize('V,pad', [(63, 3), (1029, 0), (2504, 0), (2504, 3)])
def test_target_ranks_direct(V, pad, kind):
    buf, ld = device_matrix(matrix_of(V, kind), pad)
    cubes, targets = target_rows(V)
    want = ref_scores(V, kind, 'targets', cubes)
    for rows in (len(cubes), 7):                                     # two columns per lane, and one
        cs, ts = cubes[:rows], targets[:rows]
        out = ranks_direct(buf, ld, V, cs, ts)
        assert out['rc'] == 0 and out['hits'] is None
        tp = out['tgt_ptr']
        got = [(out['ranks'][tp[r]:tp[r + 1]], out['vals'][tp[r]:tp[r + 1]]) for r in range(rows)]
        for r in range(rows):
            er, ev = G.target_ranks(want[r], cs[r], ts[r])
            assert np.array_equal(got[r][0], er), r
            assert np.array_equal(bits(got[r][1]), bits(ev)), r
            lo, hi = out['row_ptr'][r], out['row_ptr'][r + 1]
            assert np.array_equal(bits(out['cutv'][lo:hi]), bits(want[r][out['idx'][lo:hi]]))
        assert np.array_equal(np.sort(got[1][0]), np.arange(V))       # n = 0, T = V: a permutation
        assert np.array_equal(np.sort(got[3][0]), np.arange(V - 20))
        for c in np.unique(ts[4]):                                    # duplicates share their rank
            assert len(set(got[4][0][ts[4] == c].tolist())) == 1
        assert got[5][0][[1, 3, 5, 7]].tolist() == [-1, -1, -1, -1]
        assert got[5][1][[1, 3, 5, 7]].tolist() == [0.0, 0.0, 0.0, 0.0]
        assert np.all(got[5][0][[0, 2, 4, 6, 8, 9]] >= 0)
        ranks = out['ranks']
        valid = ranks[ranks >= 0]
        per_row = [ranks[tp[r]:tp[r + 1]] for r in range(rows)]
        for cutoffs in ((), (1,), (1, 10, V), (1, 2, 3, 5, 8, 13, 100, V)):       # 0, 1, 3 and 8 cut-offs
            h = ranks_direct(buf, ld, V, cs, ts, cutoffs=cutoffs, want_hits=True)
            assert h['rc'] == 0 and np.array_equal(h['ranks'], ranks)
            nk = len(cutoffs)
            assert h['hits'][:nk].tolist() == [int(np.count_nonzero(valid < K)) for K in cutoffs]
            assert h['hits'][nk] == len(valid) == sum(len(t) for t in ts) - 4     # row 5 holds 4 invalid ids
            best = sum(1 for r in per_row if np.any(r >= 0) and r[r >= 0].min() < cutoffs[0]) if nk else 0
            assert h['hits'][nk + 1] == best


def test_target_ranks_agree_with_the_device_ranking_and_splits():
    V = 1029
    rec = GraphRecommender(matrix_of(V, 'counts'))
    rng = np.random.default_rng(21)
    cubes = [rng.choice(V, int(rng.integers(0, 201)), replace=True) for _ in range(70)]
    targets = [rng.permutation(np.setdiff1d(np.arange(V), c))[:int(rng.integers(0, 40))] for c in cubes]
    full = rec.recommend_many(cubes, int(L.lib().cc_graph_rec_max_amount()))
    outs = [rec.target_ranks(cubes, targets, cutoffs=(5, 50), rows_per_launch=n) for n in (512, 64, 7)]
    a = outs[0]
    for b in outs[1:]:
        for r in range(70):
            assert np.array_equal(a[0][r], b[0][r]) and np.array_equal(bits(a[1][r]), bits(b[1][r]))
        assert np.array_equal(a[2], b[2])
    assert a[2].dtype == np.uint64 and a[2][2] == sum(len(t) for t in targets)
    for r in range(70):
        assert a[0][r].dtype == np.int32 and a[1][r].dtype == np.float64
        adds = full[r]['additions']                                   # V - n <= the cap here: the full ranking
        assert len(adds) == V - len(np.unique(cubes[r]))
        pos = np.full(V, -1, np.int64)
        pos[adds] = np.arange(len(adds))
        assert np.array_equal(a[0][r], pos[targets[r]])
        assert np.array_equal(bits(a[1][r]), bits(full[r]['add_vals'][a[0][r]]))
    assert rec.target_ranks(cubes[:2], [[], []], cutoffs=(3,))[2].tolist() == [0, 0, 0]


def test_guards():
    V = 63
    M = matrix_of(V, 'wild')
    buf, ld = device_matrix(M, 0)
    cubes = [[1, 2, 3], [4]]
    lib = L.lib()
    cap = int(lib.cc_graph_rec_max_amount())
    assert _direct(buf, ld, V, cubes, 10)['rc'] == 0
    for kw, word in ((dict(ws_shift=8), b'aligned'), (dict(null='n_add'), b'null')):
        out = _direct(buf, ld, V, cubes, 10, **kw)
        assert out['rc'] == -1 and word in lib.cc_last_error_string()      # CC_ERR_ARG
        assert np.all(out['adds'] == 77) and np.all(out['scores'] == 7.0)   # nothing launched
    out = _direct(buf, ld, V, cubes, cap + 1)
    assert out['rc'] == -1 and b'amount' in lib.cc_last_error_string() and np.all(out['adds'] == 77)
    out = _direct(buf, ld, V, cubes, 10, R=0)
    assert out['rc'] == 0 and np.all(out['adds'] == 77) and np.all(out['nadd'] == 77)
    out = ranks_direct(buf, ld, V, cubes, [[5, 6], [7]], cutoffs=(1, 2), n_cut=9)
    assert out['rc'] == -1 and b'n_cutoffs' in lib.cc_last_error_string() and np.all(out['ranks'] == 77)
    rec = GraphRecommender(M)
    with pytest.raises(ValueError, match='amount'):
        rec.recommend_many(cubes, cap + 1)
    with pytest.raises(ValueError, match='outside'):
        rec.recommend_many([[1, V]], 10)
    with pytest.raises(ValueError, match='float64'):
        GraphRecommender(M.astype(np.float32))
    assert len(rec.recommend(cubes[0], cap)['additions']) == V - 3


def test_evaluate_holdout_and_the_device_graph():
    """from_cubes builds M on the device (cc_adjacency) and the recommender reads it in place: the
    same results as over that M round-tripped through numpy, and evaluate_holdout's metrics are
    those of the reference's ranks on the oracle's M."""
    V = 300
    rng = np.random.default_rng(40)
    cubes = [rng.choice(V - 5, int(rng.integers(2, 60)), replace=True) for _ in range(40)]   # duplicates too
    lists = [np.unique(c) for c in cubes]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
    rec = GraphRecommender.from_cubes(indptr, np.concatenate(lists), V)
    M = adjacency_ref.adjacency_from_lists(lists, V)
    assert np.array_equal(bits(rec.adj.cpu().numpy()), bits(M))
    ks = (10, 50, 100)
    got = evaluate_holdout(rec, cubes, ks=ks, hide=0.2, seed=6)
    visible, hidden = holdout_split(cubes, hide=0.2, seed=6)
    want = metrics_from_ranks([G.target_ranks(G.scores(M, v), v, h)[0] for v, h in zip(visible, hidden)], ks)
    hits = got.pop('hits')
    assert got == want                                              # float64 of equal integers: equal
    assert want['n_targets'] == sum(len(h) for h in hidden) > 0
    for k, K in enumerate(ks):                                      # the device's counters say the same
        assert got[f'recall@{K}'] == hits[k] / hits[len(ks)]
    assert hits[len(ks)] == want['n_targets']
    # adjacency_device's own M against its numpy round trip
    rp, ix, C_ = upload_lists(indptr, np.concatenate(lists), V)
    Md = adjacency_device(rp, ix, C_, V, outputs=('M',))['M']
    on_device, round_trip = GraphRecommender(Md), GraphRecommender(Md.cpu().numpy())
    assert on_device.adj.data_ptr() == Md.data_ptr()
    a, b = on_device.recommend_many(cubes, 100, want_scores=True), round_trip.recommend_many(cubes, 100, want_scores=True)
    assert all(same(x, y, ('additions', 'add_vals', 'cuts', 'cut_vals', 'scores')) for x, y in zip(a, b))
    ra, rb = on_device.target_ranks(visible, hidden, cutoffs=ks), round_trip.target_ranks(visible, hidden, cutoffs=ks)
    assert all(np.array_equal(x, y) for x, y in zip(ra[0], rb[0])) and np.array_equal(ra[2], rb[2])
