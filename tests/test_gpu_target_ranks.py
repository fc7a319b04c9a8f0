"""cc_recommend_batch_target_ranks_fp32 / Recommender.target_ranks / evaluate_holdout: the exact
position of chosen target cards in each row's pinned ranking, counted on the device without
sorting.  Everything is integers or bit patterns: np.array_equal against the pinned-order CPU
oracle (the position of each target in infer_ref.top_n(p, cube, V)), no tolerances."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.evaluate import evaluate_holdout, holdout_split, metrics_from_ranks
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes
from oracle import infer_ref, model_ref
from oracle.detmath import det_sigmoid32
from tests import tile_cases

pytestmark = pytest.mark.gpu

# V below one wave slice; fewer items than threads, V no multiple of 4 x 64; several items per
# thread and more than one target chunk (2048) possible
SHAPES = [(63, 64), (1001, 128), (4100, 128)]
ALL = 30000
_models = {}
_oracle = {}


def model_of(V, d):
    if (V, d) not in _models:
        P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
        _models[(V, d)] = (P, Recommender(Layout(V, d).pack(P), V, d))
    return _models[(V, d)]


def oracle_probs(tag, P, cubes):
    """The oracle's probabilities of every cube, computed once per tag and shared."""
    if tag not in _oracle:
        _oracle[tag] = [infer_ref.recommend_probs(P, c) for c in cubes]
    return _oracle[tag]


def oracle_positions(p, cube):
    """pos[c] = position of card c in the oracle's full ranking of the candidates, -1 for a cube card."""
    V = len(p)
    adds, _ = infer_ref.top_n(p, cube, V)
    pos = np.full(V, -1, np.int64)
    pos[adds] = np.arange(len(adds))
    return pos


def expected(p, cube, targets):
    """(ranks, vals) of a target list that may hold invalid ids."""
    V = len(p)
    pos = oracle_positions(p, cube)
    t = np.asarray(targets, np.int64)
    ok = (t >= 0) & (t < V)
    ranks = np.full(len(t), -1, np.int32)
    ranks[ok] = pos[t[ok]]
    vals = np.zeros(len(t), np.float32)
    good = ranks >= 0
    vals[good] = p[t[good]]
    return ranks, vals


def mixed_batch(V):
    """(cubes, targets) of the rows the kernel's edges need; see the comments."""
    rng = np.random.default_rng(V)
    every = np.arange(V)
    cubes, targets = [], []

    def row(cube, tgt):
        cubes.append(np.asarray(cube, np.int64))
        targets.append(np.asarray(tgt, np.int64))
    row([], [])                                                     # 0: n = 0, T = 0
    row([], rng.permutation(V))                                     # 1: n = 0, T = V: a permutation
    c = rng.choice(V, 33, replace=False)
    row(c, [np.setdiff1d(every, c)[5]])                             # 2: n = 33, T = 1
    c = rng.choice(V, 20, replace=False)
    row(c, np.setdiff1d(every, c))                                  # 3: every candidate, ascending
    c = rng.choice(V, 10, replace=False)
    row(c, rng.permutation(np.setdiff1d(every, c)))                 # 4: T = V - 10, shuffled (two chunks at 4100)
    c = rng.choice(V, 15, replace=False)
    t = rng.choice(np.setdiff1d(every, c), 12, replace=False)
    row(c, rng.permutation(np.concatenate([t, t[:7], t[2:4]])))     # 5: duplicates
    c = rng.choice(V, 25, replace=False)
    t = rng.choice(np.setdiff1d(every, c), 6, replace=False)
    row(c, [t[0], c[3], t[1], V, t[2], -1, t[3], 2 ** 31 - 1, t[4], t[5]])   # 6: in the cube, = V, negative, huge
    row(rng.permutation(V), [])                                     # 7: n = V, T = 0
    c = rng.choice(V, min(V, 21), replace=False)
    t = rng.choice(np.setdiff1d(every, c), 9, replace=False)
    row(c, t)                                                       # 8, 9: identical rows
    row(c.copy(), t.copy())
    return cubes, targets


def _direct(rec, cubes, targets, cutoffs=(), want_probs=False, want_hits=None, R=None, ws_shift=0,
            null_ranks=False, n_cut=None):
    """cc_recommend_batch_target_ranks_fp32 itself, outputs and workspace pre-filled with junk."""
    V, d, dev = rec.V, rec.d, rec.dev
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    tgt_ptr = np.zeros(len(cubes) + 1, np.int32)
    tgt_ptr[1:] = np.cumsum([len(t) for t in targets])
    tgt = np.concatenate([np.asarray(t, np.int64) for t in targets]).astype(np.int32) if len(targets) else \
        np.zeros(0, np.int32)
    nt = len(tgt)
    R = len(cubes) if R is None else R
    want_hits = bool(len(cutoffs)) if want_hits is None else want_hits
    n_cut = len(cutoffs) if n_cut is None else n_cut

    def dev_of(a):
        return torch.from_numpy(a if len(a) else np.zeros(1, np.int32)).to(dev)
    rp, ix, tp, tg = dev_of(row_ptr), dev_of(idx), dev_of(tgt_ptr), dev_of(tgt)
    cut = torch.tensor(list(cutoffs) or [0], device=dev, dtype=torch.int32)
    ws = torch.full((int(L.lib().cc_recommend_batch_target_ranks_ws_size(V, d, len(cubes), max_n)) // 4 + 64,),
                    -1, device=dev, dtype=torch.int32)
    assert ws.data_ptr() % 256 == 0
    ranks = torch.full((max(nt, 1),), 77, device=dev, dtype=torch.int32)
    vals = torch.full((max(nt, 1),), 7.0, device=dev)
    hits = torch.zeros(len(cutoffs) + 2, device=dev, dtype=torch.int64) if want_hits else None
    cutv = torch.full((max(len(idx), 1),), 7.0, device=dev)
    probs = torch.full((len(cubes), V), 7.0, device=dev) if want_probs else None
    rc = L.lib().cc_recommend_batch_target_ranks_fp32(
        L.ptr(rec.params), V, d, R, L.ptr(rp), L.ptr(ix), max_n, L.ptr(tp), L.ptr(tg),
        L.ptr(cut) if len(cutoffs) else None, n_cut, L.C.c_void_p(ws.data_ptr() + ws_shift),
        None if null_ranks else L.ptr(ranks), L.ptr(vals), L.ptr(hits), L.ptr(cutv), L.ptr(probs), L.stream_ptr())
    torch.cuda.synchronize()
    return dict(rc=rc, row_ptr=row_ptr, idx=idx, tgt_ptr=tgt_ptr, ranks=ranks.cpu().numpy()[:nt],
                vals=vals.cpu().numpy()[:nt], cutv=cutv.cpu().numpy(),
                hits=hits.cpu().numpy() if want_hits else None,
                probs=probs.cpu().numpy() if want_probs else None,
                all_ranks=ranks.cpu().numpy())


@pytest.mark.parametrize('V,d', SHAPES)
def test_direct_call(V, d):
    P, rec = model_of(V, d)
    cubes, targets = mixed_batch(V)
    want = oracle_probs(('mixed', V, d), P, cubes)
    for want_probs in (False, True):
        out = _direct(rec, cubes, targets, want_probs=want_probs)   # NULL hits, n_cutoffs = 0
        assert out['rc'] == 0
        tp = out['tgt_ptr']
        got = [(out['ranks'][tp[r]:tp[r + 1]], out['vals'][tp[r]:tp[r + 1]]) for r in range(len(cubes))]
        for r, (cube, tgt) in enumerate(zip(cubes, targets)):
            er, ev = expected(want[r], cube, tgt)
            assert np.array_equal(got[r][0], er), r
            assert np.array_equal(got[r][1].view(np.uint32), ev.view(np.uint32)), r    # bit for bit
            lo, hi = out['row_ptr'][r], out['row_ptr'][r + 1]
            assert np.array_equal(out['cutv'][lo:hi], want[r][out['idx'][lo:hi]])
            if want_probs:
                assert np.array_equal(out['probs'][r], want[r])
        assert np.array_equal(np.sort(got[1][0]), np.arange(V))     # n = 0, T = V: a permutation of 0..V-1
        assert len(got[2][0]) == 1 and got[2][0][0] >= 0
        assert np.array_equal(got[3][0], oracle_positions(want[3], cubes[3])[targets[3]])
        assert np.array_equal(np.sort(got[3][0]), np.arange(V - 20))
        assert np.array_equal(np.sort(got[4][0]), np.arange(V - 10))
        assert len(targets[4]) > 2048 or V < 4100                   # more than one chunk at V = 4100
        t5 = targets[5]
        for c in np.unique(t5):                                     # duplicates share their rank
            assert len(set(got[5][0][t5 == c].tolist())) == 1
        assert got[6][0][[1, 3, 5, 7]].tolist() == [-1, -1, -1, -1]
        assert got[6][1][[1, 3, 5, 7]].tolist() == [0.0, 0.0, 0.0, 0.0]
        assert np.all(got[6][0][[0, 2, 4, 6, 8, 9]] >= 0)
        assert np.array_equal(got[8][0], got[9][0]) and np.array_equal(got[8][1], got[9][1])


@pytest.mark.parametrize('V,d,R', tile_cases.TILE_CASES)
def test_direct_call_tile_shapes(V, d, R):
    """The output tile's edges (tests/tile_cases.py) under the target-rank entry: 7 targets a row."""
    rec, cubes, want = tile_cases.recommender(V, d), tile_cases.cubes(V, R), tile_cases.probs(V, d, R)
    rng = np.random.default_rng(R)
    targets = [rng.choice(V, 7, replace=False) for _ in cubes]
    out = _direct(rec, cubes, targets, want_probs=True)
    assert out['rc'] == 0
    tp = out['tgt_ptr']
    for r, (cube, tgt) in enumerate(zip(cubes, targets)):
        er, ev = expected(want[r], cube, tgt)
        assert np.array_equal(out['ranks'][tp[r]:tp[r + 1]], er), r
        assert np.array_equal(out['vals'][tp[r]:tp[r + 1]].view(np.uint32), ev.view(np.uint32)), r
        lo, hi = out['row_ptr'][r], out['row_ptr'][r + 1]
        assert np.array_equal(out['cutv'][lo:hi], want[r][out['idx'][lo:hi]])
        assert np.array_equal(out['probs'][r], want[r])


@pytest.mark.parametrize('V,d', SHAPES)
def test_hits(V, d):
    P, rec = model_of(V, d)
    cubes, targets = mixed_batch(V)
    cutoffs = (1, 10, V)
    out = _direct(rec, cubes, targets, cutoffs=cutoffs)
    assert out['rc'] == 0
    tp, ranks, hits = out['tgt_ptr'], out['ranks'], out['hits']
    valid = ranks[ranks >= 0]
    for k, K in enumerate(cutoffs):
        assert hits[k] == np.count_nonzero(valid < K)
    assert hits[3] == len(valid) == sum(len(t) for t in targets) - 4          # row 6 holds 4 invalid ids
    assert hits[2] == hits[3]                                                   # every rank is below V
    rows = [ranks[tp[r]:tp[r + 1]] for r in range(len(cubes))]
    assert hits[4] == sum(1 for r in rows if np.any(r >= 0) and r[r >= 0].min() < cutoffs[0])
    again = _direct(rec, cubes, targets, cutoffs=cutoffs)                       # order-free totals
    assert np.array_equal(again['hits'], hits) and np.array_equal(again['ranks'], ranks)
    # the same ranks without counters; counters without cut-offs count the targets alone
    assert np.array_equal(_direct(rec, cubes, targets)['ranks'], ranks)
    bare = _direct(rec, cubes, targets, want_hits=True)
    assert bare['rc'] == 0 and bare['hits'].tolist() == [len(valid), 0]


def test_ties():
    """Long blocks of exact ones and exact zeros (the model of the ranking test's ties case):
    among equal probabilities the higher card index has the smaller rank."""
    V, d = 4100, 128
    assert det_sigmoid32(np.float32(40.0)) == np.float32(1.0)
    assert det_sigmoid32(np.float32(-200.0)) == np.float32(0.0)
    P, _ = model_of(V, d)
    P2 = dict(P)
    i = np.arange(V)
    P2['decoder/reconstruct/bias'] = np.where(i % 3 == 0, 40.0, np.where(i % 3 == 1, -200.0, -3.0)).astype(np.float32)
    rec = Recommender(Layout(V, d).pack(P2), V, d)
    cubes = [np.arange(0, 300, 7), np.zeros(0, np.int64), np.arange(V - 60, V), np.arange(0, V, 3)[5:200]]
    want = oracle_probs(('ties', V, d), P2, cubes)
    assert all(np.sum(w == 1.0) > 1000 and np.sum(w == 0.0) > 1000 for w in want)
    rng = np.random.default_rng(3)
    targets = []
    for cube, w in zip(cubes, want):
        free = np.ones(V, bool)
        free[cube] = False
        ones, zeros = np.flatnonzero((w == 1.0) & free), np.flatnonzero((w == 0.0) & free)
        targets.append(rng.permutation(np.concatenate([rng.choice(ones, 300, replace=False),
                                                       rng.choice(zeros, 300, replace=False),
                                                       ones[:2], ones[-2:], zeros[:2], zeros[-2:]])))
    ranks, vals, hits = rec.target_ranks(cubes, targets)
    assert hits is None
    for r, (cube, tgt) in enumerate(zip(cubes, targets)):
        er, ev = expected(want[r], cube, tgt)
        assert ranks[r].dtype == np.int32 and vals[r].dtype == np.float32
        assert np.array_equal(ranks[r], er) and np.array_equal(vals[r], ev)
        for tie in (1.0, 0.0):
            t, rk = tgt[vals[r] == tie], ranks[r][vals[r] == tie]
            order = np.argsort(t)
            assert np.all(np.diff(rk[order]) <= 0)                  # a higher index never ranks later
            assert np.all((np.diff(rk[order]) < 0) | (np.diff(t[order]) == 0))   # equal only for duplicates
        n_cand = V - len(cube)
        assert ranks[r][vals[r] == 0.0].max() == n_cand - 1 - 0     # zeros[0]: the very last candidate


def test_agrees_with_the_device_ranking():
    V, d = 1001, 128
    _, rec = model_of(V, d)
    rng = np.random.default_rng(21)
    cubes = [rng.choice(V, int(rng.integers(0, 201)), replace=False) for _ in range(12)]
    targets = [rng.choice(np.setdiff1d(np.arange(V), c), int(rng.integers(0, 60)), replace=False) for c in cubes]
    full = rec.recommend_many(cubes, ALL)
    ranks, vals, _ = rec.target_ranks(cubes, targets)
    for r in range(len(cubes)):
        adds = full[r]['additions']
        pos = np.full(V, -1, np.int64)
        pos[adds] = np.arange(len(adds))
        assert np.array_equal(ranks[r], pos[targets[r]])
        assert np.array_equal(vals[r], full[r]['add_vals'][ranks[r]])


def test_launch_splitting():
    V, d = 1001, 128
    P, rec = model_of(V, d)
    rng = np.random.default_rng(70)
    cubes = [rng.choice(V, int(rng.integers(0, 121)), replace=False) for _ in range(70)]
    targets = [rng.permutation(np.setdiff1d(np.arange(V), c))[:int(rng.integers(0, 40))] for c in cubes]
    outs = [rec.target_ranks(cubes, targets, cutoffs=(5, 50), rows_per_launch=n) for n in (512, 64, 7)]
    a = outs[0]
    assert len(a[0]) == len(a[1]) == 70
    for b in outs[1:]:
        for r in range(70):
            assert np.array_equal(a[0][r], b[0][r]) and np.array_equal(a[1][r], b[1][r])
        assert np.array_equal(a[2], b[2])
    assert a[2].dtype == np.uint64 and a[2][2] == sum(len(t) for t in targets)
    for r in (0, 33, 69):                                           # and they are the oracle's
        er, ev = expected(infer_ref.recommend_probs(P, cubes[r]), cubes[r], targets[r])
        assert np.array_equal(a[0][r], er) and np.array_equal(a[1][r], ev)


def test_guards():
    V, d = 63, 64
    _, rec = model_of(V, d)
    cubes, targets = [[1, 2, 3], [4]], [[5, 6], [7]]
    lib = L.lib()
    assert _direct(rec, cubes, targets)['rc'] == 0
    for kw, word in ((dict(ws_shift=4), b'aligned'), (dict(null_ranks=True), b'null'),
                     (dict(cutoffs=(1, 2), n_cut=9), b'n_cutoffs')):
        out = _direct(rec, cubes, targets, **kw)
        assert out['rc'] == -1 and word in lib.cc_last_error_string()      # CC_ERR_ARG
        assert np.all(out['all_ranks'] == 77) and np.all(out['vals'] == 7.0)   # nothing launched
    out = _direct(rec, cubes, targets, R=0)
    assert out['rc'] == 0 and np.all(out['all_ranks'] == 77)
    with pytest.raises(ValueError, match='outside'):
        rec.target_ranks(cubes, [[5, V], [7]])
    with pytest.raises(ValueError, match='outside'):
        rec.target_ranks([[1, 2, -3], [4]], targets)
    with pytest.raises(ValueError, match='cube 1: target card 4 is in the cube'):
        rec.target_ranks(cubes, [[5], [7, 4]])
    assert rec.target_ranks([], []) == ([], [], None)
    ranks, vals, hits = rec.target_ranks(cubes, [[], []], cutoffs=(3,))
    assert [len(x) for x in ranks] == [0, 0] and hits.tolist() == [0, 0, 0]


def test_evaluate_holdout_end_to_end():
    V, d = 1001, 128
    P, rec = model_of(V, d)
    rng = np.random.default_rng(40)
    cubes = [rng.choice(V, int(rng.integers(0, 201)), replace=True) for _ in range(40)]   # duplicates too
    ks = (10, 50, 100)
    got = evaluate_holdout(rec, cubes, ks=ks, hide=0.2, seed=6)
    visible, hidden = holdout_split(cubes, hide=0.2, seed=6)
    oracle_ranks = [oracle_positions(infer_ref.recommend_probs(P, v), v)[h] for v, h in zip(visible, hidden)]
    want = metrics_from_ranks(oracle_ranks, ks)
    hits = got.pop('hits')
    assert got == want                                              # float64 of equal integers: equal
    assert want['n_targets'] == sum(len(h) for h in hidden) > 0
    for k, K in enumerate(ks):                                      # the device's counters say the same
        assert got[f'recall@{K}'] == hits[k] / hits[len(ks)]
    assert hits[len(ks)] == want['n_targets']
    assert got[f'hit_rate@{ks[0]}'] == pytest.approx(hits[len(ks) + 1] / want['n_cubes'], rel=1e-15)
