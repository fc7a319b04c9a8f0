"""Diverse recommendations on the device: Recommender.recommend_diverse_many / recommend_diverse,
api.recommend_diverse and cc_recommend_diverse_fp32 itself.  The definition is the numpy float32
loop of tests/diverse_ref.py; everything is np.array_equal on ids and on the bits of the values: no
tolerances.  The shapes are the smallest at which the re-rank kernel can go wrong: candidate counts
on both sides of a wave (63, 64, 65), one candidate, the largest workgroup, rows with fewer
candidates than asked for (20 and none), as many picks as candidates, a k pad (K = 40), a table wider
than the default (K = 96), more than one launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes
from cubecobrarecommender_amd.similarity import card_embeddings, similar_many
from oracle import infer_ref, model_ref, similarity_ref
from tests import diverse_ref, tile_cases

pytestmark = pytest.mark.gpu

SHAPES = [(333, 64), (1000, 128)]
_ctx = {}


def max_candidates():
    return int(L.lib().cc_recommend_diverse_max_candidates())


def rows_of(V):
    """33 cubes: empty, one card, n on both sides of 32 and 64, unsorted input with duplicates, a
    cube that leaves 20 cards, a cube that leaves none, and random ones."""
    rng = np.random.default_rng(V)
    rows = [np.zeros(0, np.int64), np.array([V // 3])]
    rows += [rng.choice(V, n, replace=False) for n in (31, 32, 33, 63, 64, 65)]
    base = rng.choice(V, 25, replace=False)
    rows.append(rng.permutation(np.concatenate([base, base[:6]])))          # duplicates: 25 distinct
    rows.append(rng.permutation(V)[:V - 20])                                # 20 candidates
    rows.append(rng.permutation(V))                                         # no candidate
    while len(rows) < 33:
        rows.append(rng.choice(V, int(rng.integers(0, 90)), replace=False))
    return rows


def tie_columns(P, V):
    """Output columns j and j + V // 2 made equal: those two cards tie in every cube."""
    P = dict(P)
    h = V // 2
    for key in ('decoder/reconstruct/kernel', 'decoder/reconstruct/bias'):
        a = np.array(P[key], np.float32)
        a[..., h:2 * h] = a[..., :h]
        P[key] = a
    return P


class Ctx:
    """One shape's model, rows and card embeddings; recommend_many's candidates per (M, pools),
    computed once on the whole batch and shared."""

    def __init__(self, V, d, ties=False):
        self.V, self.d = V, d
        P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
        self.P = tie_columns(P, V) if ties else P
        self.rec = Recommender(Layout(V, d).pack(self.P), V, d)
        self.cubes = rows_of(V)
        self.emb = card_embeddings(self.rec).cpu().numpy()
        self._cand = {}

    def cand(self, M, pool=None, key=None):
        if (M, key) not in self._cand:
            self._cand[(M, key)] = self.rec.recommend_many(self.cubes, M, pool=pool)
        return self._cand[(M, key)]


def ctx_of(V, d, ties=False):
    if (V, d, ties) not in _ctx:
        _ctx[(V, d, ties)] = Ctx(V, d, ties)
    return _ctx[(V, d, ties)]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(got, want, cuts=None):
    ids, vals, red, rank = want
    assert got['additions'].dtype == np.int32 and got['base_rank'].dtype == np.int32
    assert got['add_vals'].dtype == np.float32 and got['redundancy'].dtype == np.float32
    assert np.array_equal(got['base_rank'], rank), (got['base_rank'], rank)
    assert np.array_equal(got['additions'], ids)
    assert np.array_equal(u32(got['add_vals']), u32(vals))
    assert np.array_equal(u32(got['redundancy']), u32(red)), (got['redundancy'], red)
    if cuts is not None:
        assert got['cut_vals'].dtype == np.float32 and np.array_equal(u32(got['cut_vals']), u32(cuts))


def check_rows(got, cands, emb, amount, trade, rows=None):
    rows = range(len(got)) if rows is None else rows
    assert len(got) == len(rows)
    for g, r in zip(got, rows):
        check(g, diverse_ref.mmr(cands[r]['additions'], cands[r]['add_vals'], emb, amount, trade), cands[r]['cut_vals'])


# ------------------------------------------------------------------------------ 1. the reference
#          trade  M      amount  rows (None: all 33)
COMBOS = [(0.0, 1, 0, None), (0.3, 63, 30, None), (0.7, 64, 64, None), (0.7, 65, 70, None), (1.0, 200, 1, None),
          (0.3, 200, 30, None), (0.7, 'max', 30, None), (0.3, 'max', 100, None),
          (0.0, 'max', 'max+5', [0, 1, 4, 8, 9, 10, 20])]


@pytest.mark.parametrize('trade,M,amount,rows', COMBOS)
@pytest.mark.parametrize('V,d', SHAPES)
def test_equals_the_reference_on_its_own_candidates(V, d, trade, M, amount, rows):
    c = ctx_of(V, d)
    M = max_candidates() if M == 'max' else M
    amount = M + 5 if amount == 'max+5' else amount
    cands = c.cand(M)
    sel = list(range(33)) if rows is None else rows
    got = c.rec.recommend_diverse_many([c.cubes[r] for r in sel], amount, trade=trade, candidates=M)
    check_rows(got, cands, c.emb, amount, trade, sel)
    by_row = dict(zip(sel, got))
    assert len(by_row[10]['additions']) == 0 and len(by_row[10]['redundancy']) == 0     # V - n = 0
    assert len(by_row[10]['cut_vals']) == V
    assert len(by_row[9]['additions']) == min(max(amount, 1), 20, M)                    # V - n = 20 < M
    assert len(by_row[0]['additions']) == min(max(amount, 1), M, V)
    if 0 < trade < 1 and M > 1 and amount > 10:
        assert any(not np.array_equal(g['base_rank'], np.arange(len(g['base_rank']))) for g in got)   # it re-ranks
        assert any(np.any(g['redundancy'] > 0) for g in got)


def test_default_arguments_and_the_single_form():
    c = ctx_of(333, 64)
    got = c.rec.recommend_diverse_many(c.cubes[:5], 30)                  # trade 0.7, max(4 * 30, 64) candidates
    check_rows(got, c.cand(120), c.emb, 30, 0.7, range(5))
    got = c.rec.recommend_diverse_many(c.cubes[:5], 5, trade=0.3)        # 64 candidates
    check_rows(got, c.cand(64), c.emb, 5, 0.3, range(5))
    one = c.rec.recommend_diverse(c.cubes[4], 30, trade=0.3, candidates=200)
    check_rows([one], c.cand(200), c.emb, 30, 0.3, [4])
    assert c.rec.recommend_diverse_many([], 30) == []
    with pytest.raises(ValueError, match='candidates'):
        c.rec.recommend_diverse_many(c.cubes[:2], 30, candidates=max_candidates() + 1)
    with pytest.raises(ValueError, match='trade'):
        c.rec.recommend_diverse(c.cubes[2], 30, trade=-0.5)


# ------------------------------------------------------------------------------ 2. the CPU oracle
@pytest.mark.parametrize('V,d,R', tile_cases.TILE_CASES)
def test_equals_the_cpu_oracle_at_the_tile_shapes(V, d, R):
    """Nothing of the GPU is in the expected values: the candidates are the oracle's probabilities
    in its ranking, the embeddings the oracle's one-card encoder rows."""
    rec, cubes = tile_cases.recommender(V, d), tile_cases.cubes(V, R)
    emb = similarity_ref.encode32_rows(tile_cases.params(V, d), np.arange(V))
    M, amount, trade = 65, 20, 0.7
    got = rec.recommend_diverse_many(cubes, amount, trade=trade, candidates=M)
    assert len(got) == R
    for cube, p, g in zip(cubes, tile_cases.probs(V, d, R), got):
        order = infer_ref.rank(p)
        free = np.ones(V, bool)
        free[cube] = False
        take = order[free[order]][:M]
        check(g, diverse_ref.mmr(take, p[take], emb, amount, trade), p[np.asarray(cube, np.int64)])


# ------------------------------------------------------------------------------ 3. synthetic tables
def table(kind, V, seed):
    rng = np.random.default_rng(seed)
    if kind.startswith('normal'):
        return rng.standard_normal((V, int(kind[6:]))).astype(np.float32)
    if kind == 'groups':                        # identical rows: sim ties and the greatest redundancy
        return rng.standard_normal((37, 64)).astype(np.float32)[np.arange(V) % 37]
    if kind == 'zeros':
        return np.zeros((V, 64), np.float32)
    assert kind == 'onehot'                     # sims exactly 0 or 1 (powers of two normalise exactly)
    e = np.zeros((V, 64), np.float32)
    e[np.arange(V), rng.integers(0, 64, V)] = np.exp2(rng.integers(-10, 11, V)).astype(np.float32)
    return e


@pytest.mark.parametrize('kind', ['normal64', 'normal40', 'normal96', 'normal5', 'groups', 'zeros', 'onehot'])
def test_synthetic_embeddings(kind):
    V, d = 333, 64
    c = ctx_of(V, d)
    e = table(kind, V, seed=len(kind))
    M, amount = 200, 60
    cands = c.cand(M)
    for trade, emb in ((0.3, torch.from_numpy(e).cuda()), (0.7, e)):     # a device tensor, a host array
        got = c.rec.recommend_diverse_many(c.cubes, amount, trade=trade, candidates=M, emb=emb)
        check_rows(got, cands, e, amount, trade)
        for g in got:
            if kind == 'zeros':
                assert np.array_equal(g['base_rank'], np.arange(len(g['base_rank']))) and np.all(u32(g['redundancy']) == 0)
            if kind == 'onehot':
                assert set(u32(g['redundancy']).tolist()) <= {0, 0x3F800000}
        if kind == 'groups':
            assert any(np.any(g['redundancy'] > 0.999) for g in got)
        if kind == 'onehot':
            assert any(0x3F800000 in u32(g['redundancy']) for g in got)


def test_similarity_is_similar_manys_negated_distance():
    """trade 0: the first pick is candidate 0, and the second is charged its similarity to it."""
    c = ctx_of(333, 64)
    got = c.rec.recommend_diverse_many(c.cubes[:9], 2, trade=0.0, candidates=64)
    emb = card_embeddings(c.rec)
    for g in got:
        a, b = g['additions'].tolist()
        idx, dist = similar_many(emb, [a], c.V)
        at = int(np.flatnonzero(idx[0] == b)[0])
        sim = np.float32(-dist[0, at])
        assert u32(g['redundancy'])[1] == u32(np.array([sim if sim > 0 else 0], np.float32))[0]


# ------------------------------------------------------------------------------ 4. ties in p
def test_ties_in_p_follow_the_base_order():
    V, d = 333, 64
    c = ctx_of(V, d, ties=True)
    M = 100
    cands = c.cand(M)
    assert sum(int(np.any(o['add_vals'][1:] == o['add_vals'][:-1])) for o in cands) > 20
    for trade in (0.3, 1.0):
        check_rows(c.rec.recommend_diverse_many(c.cubes, 40, trade=trade, candidates=M), cands, c.emb, 40, trade)
    flat = c.rec.recommend_diverse_many(c.cubes, M, trade=0.5, candidates=M, emb=np.zeros((V, 64), np.float32))
    for g, o in zip(flat, cands):
        assert np.array_equal(g['additions'], o['additions']) and np.array_equal(u32(g['add_vals']), u32(o['add_vals']))


# ------------------------------------------------------------------------------ 5. trade = 1
@pytest.mark.parametrize('V,d', SHAPES)
def test_trade_one_is_recommend_many(V, d):
    c = ctx_of(V, d)
    pool = c.rec.card_pool(np.arange(0, V, 3))
    for amount, M in ((30, 30), (30, 64), (1, max_candidates()), (100, max_candidates())):
        for p in (None, pool):
            want = c.rec.recommend_many(c.cubes, amount, pool=p)
            got = c.rec.recommend_diverse_many(c.cubes, amount, trade=1.0, candidates=M, pool=p)
            for g, w in zip(got, want):
                assert np.array_equal(g['additions'], w['additions'])
                assert np.array_equal(u32(g['add_vals']), u32(w['add_vals']))
                assert np.array_equal(u32(g['cut_vals']), u32(w['cut_vals']))
                assert np.array_equal(g['base_rank'], np.arange(len(w['additions'])))
                assert np.all(u32(g['redundancy'][:1]) == 0)


# ------------------------------------------------------------------------------ 6. pools
def test_pools():
    V, d = 333, 64
    c = ctx_of(V, d)
    rng = np.random.default_rng(9)
    even = c.rec.card_pool(np.arange(0, V, 2))
    few = c.rec.card_pool(rng.choice(V, 25, replace=False))
    per_row = [(even, None, few)[r % 3] for r in range(33)]
    M, amount, trade = 100, 30, 0.7
    for pool, key in ((even, 'even'), (per_row, 'per row')):
        cands = c.cand(M, pool=pool, key=key)
        got = c.rec.recommend_diverse_many(c.cubes, amount, trade=trade, candidates=M, pool=pool)
        check_rows(got, cands, c.emb, amount, trade)
        for r, g in enumerate(got):
            p = pool if key == 'even' else per_row[r]
            if p is not None:
                assert np.all(p.contains(g['additions']))
            assert not set(g['additions'].tolist()) & set(np.asarray(c.cubes[r]).tolist())
    assert any(0 < len(g['additions']) < amount for g, p in zip(got, per_row) if p is few)   # the pool ran out
    check_rows([got[1]], c.cand(M), c.emb, amount, trade, [1])                               # a row without one


# ------------------------------------------------------------------------------ 7. batch independence
def test_batch_independence():
    c = ctx_of(1000, 128)
    M, amount, trade = 130, 40, 0.3
    cands = c.cand(M)
    for rows in (1, 7, 512):
        check_rows(c.rec.recommend_diverse_many(c.cubes, amount, trade=trade, candidates=M, rows_per_launch=rows),
                   cands, c.emb, amount, trade)
    for r in (0, 1, 9, 10, 32):
        check_rows(c.rec.recommend_diverse_many([c.cubes[r]], amount, trade=trade, candidates=M), cands, c.emb,
                   amount, trade, [r])
    twins = c.rec.recommend_diverse_many([c.cubes[4], c.cubes[10], c.cubes[4].copy()], amount, trade=trade,
                                         candidates=M)
    check_rows(twins, cands, c.emb, amount, trade, [4, 10, 4])


# ------------------------------------------------------------------------------ 8. the C entry
JUNK_I, JUNK_F = 77, 7.0


def _direct(rec, cubes, amount, M, lam, emb, extra=3, pool_words=None, pool_of_row=None, ws_shift=0, over=None):
    V, d, dev = rec.V, rec.d, rec.dev
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    R, K = len(cubes), emb.shape[1]
    A = min(max(amount, 1), M) + extra                              # a pitch above the need: a tail in every row
    rp = torch.from_numpy(row_ptr).to(dev)
    ix = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(dev)
    emb_d = torch.from_numpy(np.ascontiguousarray(emb, np.float32)).to(dev)
    ws = torch.full((int(L.lib().cc_recommend_diverse_ws_size(V, d, R, max_n, M, K)) // 4 + 64,), -1, device=dev,
                    dtype=torch.int32)
    assert ws.data_ptr() % 256 == 0
    nadd = torch.full((R,), JUNK_I, device=dev, dtype=torch.int32)
    adds = torch.full((R, A), JUNK_I, device=dev, dtype=torch.int32)
    rank = torch.full((R, A), JUNK_I, device=dev, dtype=torch.int32)
    addv = torch.full((R, A), JUNK_F, device=dev)
    red = torch.full((R, A), JUNK_F, device=dev)
    cuts = torch.full((max(len(idx), 1),), JUNK_F, device=dev)
    table = por = None
    if pool_words is not None:
        table = torch.from_numpy(np.stack(pool_words).view(np.int32)).to(dev)
        por = torch.tensor(pool_of_row, device=dev, dtype=torch.int32)
    args = dict(params=L.ptr(rec.params), V=V, d=d, R=R, row_ptr=L.ptr(rp), idx=L.ptr(ix), max_n=max_n, amount=amount,
                M=M, lam=lam, emb=L.ptr(emb_d), K=K, pools=L.ptr(table),
                n_pools=0 if pool_words is None else len(pool_words), pool_of_row=L.ptr(por), A=A, n_add=L.ptr(nadd),
                additions=L.ptr(adds), add_vals=L.ptr(addv), redundancy=L.ptr(red), base_rank=L.ptr(rank),
                cut_vals=L.ptr(cuts), ws=C.c_void_p(ws.data_ptr() + ws_shift), ws_bytes=ws.numel() * 4 - ws_shift,
                stream=L.stream_ptr())
    args.update(over or {})
    rc = L.lib().cc_recommend_diverse_fp32(*args.values())
    torch.cuda.synchronize()
    return dict(rc=rc, nadd=nadd.cpu().numpy(), adds=adds.cpu().numpy(), addv=addv.cpu().numpy(),
                red=red.cpu().numpy(), rank=rank.cpu().numpy(), cuts=cuts.cpu().numpy(), ws=ws.cpu().numpy(),
                row_ptr=rp.cpu().numpy(), idx=ix.cpu().numpy())


def _untouched(out):
    return (np.all(out['nadd'] == JUNK_I) and np.all(out['adds'] == JUNK_I) and np.all(out['rank'] == JUNK_I)
            and np.all(out['addv'] == JUNK_F) and np.all(out['red'] == JUNK_F) and np.all(out['cuts'] == JUNK_F)
            and np.all(out['ws'] == -1))


@pytest.mark.parametrize('K,M', [(64, 130), (96, 341), (40, 64)])
def test_direct_call(K, M):
    c = ctx_of(333, 64)
    sel = list(range(14))
    cubes = [c.cubes[r] for r in sel]
    e = c.emb if K == 64 else table(f'normal{K}', c.V, seed=K)
    amount, lam = 50, 0.3
    cands = c.cand(M)
    row_ptr, idx, _, _, slot = pack_cubes(cubes, c.V)
    out = _direct(c.rec, cubes, amount, M, lam, e)
    assert out['rc'] == 0
    assert np.array_equal(out['row_ptr'], row_ptr) and np.array_equal(out['idx'], idx)         # inputs not written
    for i, r in enumerate(sel):
        ids, vals, red, rank = diverse_ref.mmr(cands[r]['additions'], cands[r]['add_vals'], e, amount, lam)
        k = out['nadd'][i]
        assert k == len(ids) and out['adds'].shape[1] > k                                       # a tail to check
        assert np.array_equal(out['adds'][i, :k], ids) and np.array_equal(out['rank'][i, :k], rank)
        assert np.array_equal(u32(out['addv'][i, :k]), u32(vals)) and np.array_equal(u32(out['red'][i, :k]), u32(red))
        assert np.all(out['adds'][i, k:] == JUNK_I) and np.all(out['rank'][i, k:] == JUNK_I)   # left as they were
        assert np.all(out['addv'][i, k:] == JUNK_F) and np.all(out['red'][i, k:] == JUNK_F)
        lo, hi = row_ptr[i], row_ptr[i + 1]
        want_cuts = np.zeros(hi - lo, np.float32)
        n_in = len(cubes[i])
        at = int(sum(len(x) for x in cubes[:i]))
        want_cuts[slot[at:at + n_in] - lo] = cands[r]['cut_vals']
        assert np.array_equal(u32(out['cuts'][lo:hi]), u32(want_cuts))
    assert out['nadd'][10] == 0 and out['nadd'][9] == 20


def test_direct_call_pools_and_no_rows():
    c = ctx_of(333, 64)
    sel = list(range(12))
    cubes = [c.cubes[r] for r in sel]
    ids = np.arange(0, c.V, 2)
    even = np.zeros((c.V + 31) // 32, np.uint32)
    np.bitwise_or.at(even, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    por = [(0, -1, 1)[i % 3] for i in sel]                         # pool 0, none, no pool of the table: no candidates
    M, amount, lam = 64, 20, 0.7
    out = _direct(c.rec, cubes, amount, M, lam, c.emb, pool_words=[even], pool_of_row=por)
    assert out['rc'] == 0
    pool = c.rec.card_pool(ids)
    cands = c.rec.recommend_many(cubes, M, pool=[(pool, None, None)[i % 3] for i in sel])
    for i in sel:
        k = out['nadd'][i]
        if por[i] == 1:
            assert k == 0 and np.all(out['adds'][i] == JUNK_I)
            continue
        want = diverse_ref.mmr(cands[i]['additions'], cands[i]['add_vals'], c.emb, amount, lam)
        assert k == len(want[0]) and np.array_equal(out['adds'][i, :k], want[0])
        assert np.array_equal(u32(out['red'][i, :k]), u32(want[2]))
    out = _direct(c.rec, cubes, amount, M, lam, c.emb, over=dict(R=0))
    assert out['rc'] == 0 and _untouched(out)


def test_guards_write_nothing():
    c = ctx_of(333, 64)
    cubes = c.cubes[:6]
    lib = L.lib()
    top = max_candidates()
    wide = table('normal96', c.V, seed=96)
    cases = [(dict(ws_shift=4), b'aligned'), (dict(over=dict(ws_bytes=1024)), b'workspace'),
             (dict(over=dict(lam=-0.25)), b'lambda'), (dict(over=dict(lam=1.5)), b'lambda'),
             (dict(over=dict(lam=float('nan'))), b'lambda'), (dict(over=dict(M=0)), b'M outside'),
             (dict(over=dict(M=top + 1)), b'M outside'), (dict(over=dict(A=19)), b'A below'),
             (dict(over=dict(emb=None)), b'null'), (dict(over=dict(redundancy=None)), b'null'),
             (dict(over=dict(base_rank=None)), b'null'), (dict(over=dict(cut_vals=None)), b'null'),
             (dict(over=dict(K=0)), b'K'), (dict(over=dict(max_n=c.V + 1)), b'max_n'),
             (dict(over=dict(n_pools=1)), b'null')]
    for kw, word in cases:
        out = _direct(c.rec, cubes, 20, 64, 0.5, c.emb, **kw)
        assert out['rc'] == -1 and b'cc_recommend_diverse_fp32' in lib.cc_last_error_string(), kw
        assert word in lib.cc_last_error_string() and _untouched(out), kw
    out = _direct(c.rec, cubes, 20, 342, 0.5, wide)                 # 96 floats: at most 341 candidates
    assert out['rc'] == -1 and b'LDS' in lib.cc_last_error_string() and _untouched(out)


# ------------------------------------------------------------------------------ 9. api
def test_api_json_shape():
    V, d = 333, 64
    c = ctx_of(V, d)

    class Model:
        def recommender(self):
            return c.rec
    names = {i: f'card {i}' for i in range(V)}
    cube = [5, 9, 5, 40, 2]
    for trade, cand, pool in ((0.7, None, None), (0.3, 90, c.rec.card_pool(np.arange(1, V, 2)))):
        got = api.recommend_diverse(Model(), iter(cube), 12, names, trade=trade, candidates=cand, pool=pool)
        base = c.rec.recommend_many([cube], 64 if cand is None else cand, pool=pool)[0]
        ids, vals, red, rank = diverse_ref.mmr(base['additions'], base['add_vals'], c.emb, 12, trade)
        assert list(got) == ['additions', 'redundancy', 'base_rank']
        want_names = [names[i] for i in ids.tolist()]
        for key, col in (('additions', vals), ('redundancy', red), ('base_rank', rank)):
            assert list(got[key]) == want_names and list(got[key].values()) == col.tolist()     # in pick order
        assert all(type(v) is float for v in got['additions'].values())
        assert all(type(v) is int for v in got['base_rank'].values())
        assert len(got['additions']) == 12
