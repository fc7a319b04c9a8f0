"""Card pools on the batched recommend path: recommend_many / recommend / target_ranks with pool=
and the three cc_recommend_batch_*pool*_fp32 entries.  A pooled row's additions are the members of
pool minus cube, in the order and with the bits of the row's unpooled ranking; cut values and
probabilities do not depend on the pool.  Everything is np.array_equal against the pinned-order CPU
oracle (infer_ref.rank of infer_ref.recommend_probs, filtered on the host): no tolerances."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import CardPool, Recommender, pack_cubes
from oracle import infer_ref, model_ref
from tests import tile_cases

pytestmark = pytest.mark.gpu

# the degenerate row; a partial last mask word (31 and 9 valid bits) and exactly whole words;
# V - n above the select's 2048 survivors with several items per thread
SHAPES = [(1, 64), (63, 64), (64, 64), (1001, 128), (4100, 128)]
ALL = 30000                                            # the web endpoint's default: above every V
CUBE_ROW = 5                                           # the mixed batch's row whose cube is a pool
ROW_SETS = {'R11': slice(0, 11), 'R33': slice(0, 33), 'R70': slice(11, 81)}   # out_tile_kernel<2 / 4 / 8>
_ctx = {}


def cap():
    return int(L.lib().cc_recommend_batch_max_amount())


def amounts(V):
    return [0, 1, 7, cap(), cap() + 1, V, ALL]


def mixed_batch(V):
    """11 rows: n = 0, 1, 32, 33, 65, min(V, 500), V - 1, V (each capped at V); one row unsorted
    with duplicates; two identical rows."""
    rng = np.random.default_rng(V)
    cubes = [rng.choice(V, min(n, V), replace=False) for n in (0, 1, 32, 33, 65, min(V, 500), V - 1, V)]
    base = rng.choice(V, min(V, 40), replace=False)
    cubes.append(rng.permutation(np.concatenate([base, base[:9], base[3:5]])))
    twin = rng.choice(V, min(V, 21), replace=False)
    cubes += [twin, twin.copy()]
    return cubes


def random_cubes(V, R, seed):
    rng = np.random.default_rng(seed)
    return [rng.choice(V, min(V, int(rng.integers(0, 201))), replace=False) for _ in range(R)]


def pool_ids(V, cubes):
    rng = np.random.default_rng(1000 + V)
    cube = np.unique(cubes[CUBE_ROW])
    return {
        'empty': np.zeros(0, np.int64),
        'first': np.array([0]),
        'last': np.array([V - 1]),
        'all': np.arange(V),
        'last_word': np.arange(32 * ((V - 1) // 32), V),
        'every_other': np.arange(0, V, 2),
        'two_percent': rng.choice(V, max(1, V // 50), replace=False),
        'cube': cube,
        'not_cube': np.setdiff1d(np.arange(V), cube),
    }


class Ctx:
    """One shape's model, rows, oracle probabilities / rankings and pools: computed once, shared,
    never changed."""

    def __init__(self, V, d, ties=False):
        self.V, self.d = V, d
        P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
        self.cubes = mixed_batch(V) + random_cubes(V, 70, seed=V + 7)
        if ties:                                       # every probability takes one of three values
            P = dict(P)
            P['decoder/reconstruct/kernel'] = np.zeros_like(P['decoder/reconstruct/kernel'])
            P['decoder/reconstruct/bias'] = np.choose(np.arange(V) % 3, [2.0, 0.0, -3.0]).astype(np.float32)
            self.cubes = self.cubes[:33]
        self.P = P
        self.rec = Recommender(Layout(V, d).pack(P), V, d)
        self.p = [infer_ref.recommend_probs(P, c) for c in self.cubes]
        self.order = [infer_ref.rank(p) for p in self.p]
        self.in_cube = []
        for c in self.cubes:
            m = np.zeros(V, bool)
            m[np.asarray(c, np.int64)] = True
            self.in_cube.append(m)
        self.ids = pool_ids(V, self.cubes)
        self.pools = {k: self.rec.card_pool(v) for k, v in self.ids.items()}
        self.member = {None: np.ones(V, bool)}
        for k, v in self.ids.items():
            self.member[k] = np.zeros(V, bool)
            self.member[k][v] = True
        names = ['every_other', None, 'two_percent', 'not_cube', 'last_word']
        rng = np.random.default_rng(V + 99)
        self.mix_names = [names[i] for i in rng.integers(0, len(names), len(self.cubes))]
        self.mix_names[CUBE_ROW] = 'cube'              # no candidates here, its neighbours have some
        self.mix_names[CUBE_ROW - 1], self.mix_names[CUBE_ROW + 1] = 'every_other', None
        self._cand = {}

    def cand(self, r, name):
        """Row r's candidates with pool `name` (None: no pool), in the oracle's ranking order."""
        if (r, name) not in self._cand:
            o = self.order[r]
            self._cand[(r, name)] = o[self.member[name][o] & ~self.in_cube[r][o]]
        return self._cand[(r, name)]

    def pool_arg(self, name, rows):
        if name == 'mix':
            return [None if n is None else self.pools[n] for n in self.mix_names[rows]]
        return self.pools[name]

    def name_of(self, name, r):
        return self.mix_names[r] if name == 'mix' else name


def ctx_of(V, d, ties=False):
    if (V, d, ties) not in _ctx:
        _ctx[(V, d, ties)] = Ctx(V, d, ties)
    return _ctx[(V, d, ties)]


def check_row(out, p, cube, cand, amount, probs=False):
    exp = cand[:max(int(amount), 1)]
    assert out['additions'].dtype == np.int32 and out['add_vals'].dtype == np.float32
    assert out['cut_vals'].dtype == np.float32
    assert np.array_equal(out['additions'], exp)                    # n_add is the length of that list
    assert np.array_equal(out['add_vals'], p[exp])
    assert np.array_equal(out['cut_vals'], p[np.asarray(cube, np.int64)])   # input order, duplicates kept
    if probs:
        assert np.array_equal(out['probs'], p)


POOL_NAMES = ['empty', 'first', 'last', 'all', 'last_word', 'every_other', 'two_percent', 'cube', 'not_cube', 'mix']


@pytest.mark.parametrize('rows', list(ROW_SETS))
@pytest.mark.parametrize('V,d', SHAPES)
def test_pools_bit_exact(V, d, rows):
    c = ctx_of(V, d)
    sl = ROW_SETS[rows]
    idx = range(*sl.indices(len(c.cubes)))
    cubes = c.cubes[sl]
    for name in POOL_NAMES:
        for amount in amounts(V):
            probs = amount == 7
            outs = c.rec.recommend_many(cubes, amount, want_probs=probs, pool=c.pool_arg(name, sl))
            assert len(outs) == len(cubes)
            for out, r in zip(outs, idx):
                check_row(out, c.p[r], c.cubes[r], c.cand(r, c.name_of(name, r)), amount, probs=probs)
    if sl.start == 0:                                               # the row whose cube is its pool
        outs = c.rec.recommend_many(cubes, ALL, pool=c.pool_arg('mix', sl))
        assert len(outs[CUBE_ROW]['additions']) == 0
        assert len(outs[CUBE_ROW + 1]['additions']) == 1           # n = V - 1 and no pool: one candidate
        if V >= 1001:
            assert len(outs[CUBE_ROW - 1]['additions']) > 0


@pytest.mark.parametrize('V,d,R', tile_cases.TILE_CASES)
def test_pools_tile_shapes(V, d, R):
    """The pooled output tile's edges (tests/tile_cases.py): every other card allowed."""
    rec, cubes, want = tile_cases.recommender(V, d), tile_cases.cubes(V, R), tile_cases.probs(V, d, R)
    allowed = np.arange(V) % 2 == 0
    outs = rec.recommend_many(cubes, 7, want_probs=True, pool=rec.card_pool(np.flatnonzero(allowed)))
    assert len(outs) == R
    for r, cube in enumerate(cubes):
        ok = allowed.copy()
        ok[cube] = False
        o = infer_ref.rank(want[r])
        check_row(outs[r], want[r], cube, o[ok[o]], 7, probs=True)


@pytest.mark.parametrize('V,d', SHAPES)
def test_ties(V, d):
    """A zero output kernel and a bias cycling through three values: every probability is one of
    three, whole tie blocks lie across the pool boundary and across the `amount` cut."""
    c = ctx_of(V, d, ties=True)
    R = len(c.cubes)
    assert all(len(np.unique(p)) == min(3, V) for p in c.p)
    # the oracle alone: a candidate tie block straddles the cut (and has members outside the pool)
    for amount in (7, cap()):
        hit = 0
        for name in ('every_other', 'not_cube', 'all', 'mix'):
            for r in range(R):
                cand, p = c.cand(r, c.name_of(name, r)), c.p[r]
                if len(cand) > amount and p[cand[amount - 1]] == p[cand[amount]]:
                    free = ~c.in_cube[r]
                    if name != 'all' and not np.any(free & ~c.member[c.name_of(name, r)] & (p == p[cand[amount]])):
                        continue
                    hit += 1
        if V >= 63 and (amount == 7 or V > 2 * cap()):
            assert hit > 0, (V, amount)
    for name in ('every_other', 'not_cube', 'all', 'two_percent', 'last_word', 'mix'):
        for amount in amounts(V):
            outs = c.rec.recommend_many(c.cubes, amount, pool=c.pool_arg(name, slice(0, R)))
            for r, out in enumerate(outs):
                check_row(out, c.p[r], c.cubes[r], c.cand(r, c.name_of(name, r)), amount)
                adds, vals = out['additions'], out['add_vals']
                same = vals[1:] == vals[:-1]
                assert np.all(np.diff(adds)[same] < 0)              # equal values: higher card index first


def same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize('V,d', SHAPES)
def test_invariants(V, d):
    c = ctx_of(V, d)
    rec, cubes = c.rec, c.cubes
    R = len(cubes)
    whole = slice(0, R)
    for amount in (7, cap() + 1):
        plain = rec.recommend_many(cubes, amount, want_probs=True)
        for pool in (None, [None] * R, c.pools['all']):            # no pool at all; the pool of all cards
            got = rec.recommend_many(cubes, amount, want_probs=True, pool=pool)
            for r in range(R):
                same(got[r], plain[r])
        mix = c.pool_arg('mix', whole)
        a = rec.recommend_many(cubes, amount, want_probs=True, pool=mix, rows_per_launch=512)
        b = rec.recommend_many(cubes, amount, want_probs=True, pool=mix, rows_per_launch=7)
        for r in range(R):
            same(a[r], b[r])                                        # the launch a row falls into
        # a row's neighbours and their pools: alone, and among rows that all share its pool
        for r in (0, 3, CUBE_ROW, 8, 40, R - 1):
            alone = rec.recommend_many([cubes[r]], amount, want_probs=True, pool=mix[r])[0]
            same(alone, a[r])
            if mix[r] is not None and r < 12:
                among = rec.recommend_many(cubes[:12], amount, want_probs=True, pool=mix[r])
                same(among[r], a[r])
            one = rec.recommend(cubes[r], amount, want_probs=True, pool=mix[r])
            same(one, a[r])
        for name in ('every_other', 'cube', 'empty'):               # recommend(pool=) is row 0 of recommend_many
            many = rec.recommend_many(cubes[:3], amount, pool=c.pools[name])
            same(rec.recommend(cubes[0], amount, pool=c.pools[name]), many[0])
    with pytest.raises(ValueError, match='want_order'):
        rec.recommend(cubes[0], 7, want_order=True, pool=c.pools['all'])
    host_only = CardPool(c.ids['every_other'], V)                   # a pool that was never uploaded
    got = rec.recommend_many(cubes[:11], 7, pool=host_only)
    want = rec.recommend_many(cubes[:11], 7, pool=c.pools['every_other'])
    for r in range(11):
        same(got[r], want[r])


def targets_of(c, name, seed):
    """Per row: a shuffled sample of its candidates with a few duplicates; every candidate for some rows."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(len(c.cubes)):
        cand = c.cand(r, c.name_of(name, r))
        if r % 9 == 2 or len(cand) == 0:
            t = rng.permutation(cand)
        else:
            t = rng.choice(cand, min(len(cand), int(rng.integers(0, 40))), replace=False)
            t = np.concatenate([t, t[:3]])
        out.append(np.asarray(t, np.int64))
    return out


@pytest.mark.parametrize('V,d', SHAPES)
def test_target_ranks(V, d):
    c = ctx_of(V, d)
    rec, cubes = c.rec, c.cubes
    R = len(cubes)
    cutoffs = (1, 5, 50)
    for name in ('every_other', 'two_percent', 'mix'):
        pool = c.pool_arg(name, slice(0, R))
        targets = targets_of(c, name, seed=V + len(name))
        full = rec.recommend_many(cubes, V, pool=pool)              # the pooled additions at amount = V
        for rows_per_launch in (512, 7):
            ranks, vals, hits = rec.target_ranks(cubes, targets, cutoffs=cutoffs, pool=pool,
                                                 rows_per_launch=rows_per_launch)
            assert len(ranks) == len(vals) == R
            for r in range(R):
                adds = full[r]['additions']
                assert np.array_equal(adds, c.cand(r, c.name_of(name, r)))
                pos = np.full(V, -1, np.int64)
                pos[adds] = np.arange(len(adds))
                assert ranks[r].dtype == np.int32 and vals[r].dtype == np.float32
                assert np.array_equal(ranks[r], pos[targets[r]]) and np.all(ranks[r] >= 0)
                assert np.array_equal(vals[r], c.p[r][targets[r]])
            allr = np.concatenate(ranks)
            want = [np.count_nonzero(allr < K) for K in cutoffs] + [len(allr)]
            want.append(sum(1 for r in ranks if len(r) and r.min() < cutoffs[0]))
            assert hits.dtype == np.uint64 and hits.tolist() == want
    odd_free = np.setdiff1d(np.flatnonzero(~c.in_cube[2]), c.ids['every_other'])
    if len(odd_free):                                               # a candidate of the row, but not of its pool
        with pytest.raises(ValueError, match=f'cube 2: target card {odd_free[0]} is outside the pool'):
            rec.target_ranks(cubes[:3], [[], [], [odd_free[0]]], pool=c.pools['every_other'])
    with pytest.raises(ValueError, match='cube 0: target card 0 is outside the pool'):
        rec.target_ranks([[]], [[0]], pool=c.pools['empty'])


def test_api_json_shapes():
    from cubecobrarecommender_amd import api
    V, d = 63, 64
    c = ctx_of(V, d)

    class Model:
        def recommender(self):
            return c.rec
    names = {i: f'card {i}' for i in range(V)}
    cubes = [[int(i) for i in cube] for cube in c.cubes[:4]]
    pool = c.pools['every_other']
    many = api.recommend_many(Model(), cubes, 5, names, pool=pool)
    assert len(many) == 4
    for r, (cube, got) in enumerate(zip(cubes, many)):
        exp = c.cand(r, 'every_other')[:5]
        assert list(got['additions']) == [names[i] for i in exp]            # best first
        assert list(got['additions'].values()) == c.p[r][exp].tolist()
        assert got['cuts'] == {names[i]: float(c.p[r][i]) for i in cube}    # every cube card, pool or not
        assert api.recommend(Model(), cube, 5, names, pool=pool) == got
    assert api.recommend_many(Model(), cubes, 5, names) == api.recommend_many(Model(), cubes, 5, names, pool=None)


# ---------------------------------------------------------------------------------- direct C calls
def _direct(rec, cubes, amount, entry, pools, pool_of_row, n_pools=None, null_pools=False, ws_shift=0,
            null_rows=False):
    """cc_recommend_batch_pool_fp32 / cc_recommend_batch_rank_pool_fp32 themselves, outputs and
    workspace pre-filled with junk."""
    V, d, dev = rec.V, rec.d, rec.dev
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    R = len(cubes)
    A = max(amount, 1) if entry == 'cc_recommend_batch_pool' else min(max(amount, 1), V)
    rp = torch.from_numpy(row_ptr).to(dev)
    ix = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(dev)
    table = torch.from_numpy(np.stack(pools).view(np.int32)).to(dev)
    por = torch.tensor(pool_of_row, device=dev, dtype=torch.int32)
    ws = torch.full((int(getattr(L.lib(), entry + '_ws_size')(V, d, R, max_n)) // 4 + 64,), -1,
                    device=dev, dtype=torch.int32)
    assert ws.data_ptr() % 256 == 0
    nadd = torch.full((R,), 77, device=dev, dtype=torch.int32)
    adds = torch.full((R, A), 77, device=dev, dtype=torch.int32)
    addv = torch.full((R, A), 7.0, device=dev)
    cutv = torch.full((max(len(idx), 1),), 7.0, device=dev)
    rc = getattr(L.lib(), entry + '_fp32')(
        L.ptr(rec.params), V, d, R, L.ptr(rp), L.ptr(ix), max_n, amount,
        L.C.c_void_p(ws.data_ptr() + ws_shift), L.ptr(nadd), L.ptr(adds), L.ptr(addv), L.ptr(cutv), None,
        None if null_pools else L.ptr(table), len(pools) if n_pools is None else n_pools,
        None if null_rows else L.ptr(por), L.stream_ptr())
    torch.cuda.synchronize()
    return dict(rc=rc, row_ptr=row_ptr, idx=idx, nadd=nadd.cpu().numpy(), adds=adds.cpu().numpy(),
                addv=addv.cpu().numpy(), cutv=cutv.cpu().numpy())


@pytest.mark.parametrize('entry', ['cc_recommend_batch_pool', 'cc_recommend_batch_rank_pool'])
@pytest.mark.parametrize('V,d', [(63, 64), (1001, 128)])
def test_direct_call(V, d, entry):
    c = ctx_of(V, d)
    rows = list(range(11))
    cubes = [c.cubes[r] for r in rows]
    words = [c.pools['every_other'].words, c.pools['two_percent'].words]
    #              pool 0, none, pool 1, = n_pools, -7, then pools 0 / 1 / none in turn
    pool_of_row = [0, -1, 1, 2, -7, 0, 1, -1, 0, 1, -1]
    names = {0: 'every_other', 1: 'two_percent', -1: None}
    lib = L.lib()
    for amount in (0, 7, V, ALL if entry.endswith('rank_pool') else cap()):
        out = _direct(c.rec, cubes, amount, entry, words, pool_of_row)
        assert out['rc'] == 0
        A = out['adds'].shape[1]
        assert A == (min(max(amount, 1), V) if entry.endswith('rank_pool') else max(amount, 1))
        for r in rows:
            k = out['nadd'][r]
            if pool_of_row[r] in (2, -7):                           # not a pool of the table: no candidates
                exp = np.zeros(0, np.int64)
            else:
                exp = c.cand(r, names[pool_of_row[r]])[:max(amount, 1)]
            assert k == len(exp)
            assert np.array_equal(out['adds'][r, :k], exp) and np.array_equal(out['addv'][r, :k], c.p[r][exp])
            assert np.all(out['adds'][r, k:] == -1) and np.all(out['addv'][r, k:] == 0.0)
            lo, hi = out['row_ptr'][r], out['row_ptr'][r + 1]
            assert np.array_equal(out['cutv'][lo:hi], c.p[r][out['idx'][lo:hi]])
    # no pool at all: pools NULL with n_pools == 0 is legal, every row unpooled
    out = _direct(c.rec, cubes, 7, entry, words, [-1] * 11, n_pools=0, null_pools=True)
    assert out['rc'] == 0
    for r in rows:
        assert np.array_equal(out['adds'][r, :out['nadd'][r]], c.cand(r, None)[:7])
    for kw, word in ((dict(null_pools=True), b'pools is null'), (dict(n_pools=-1), b'n_pools'),
                     (dict(null_rows=True), b'null'), (dict(ws_shift=4), b'aligned')):
        out = _direct(c.rec, cubes, 7, entry, words, pool_of_row, **kw)
        assert out['rc'] == -1 and word in lib.cc_last_error_string()          # CC_ERR_ARG
        assert np.all(out['nadd'] == 77) and np.all(out['adds'] == 77) and np.all(out['addv'] == 7.0)
        assert np.all(out['cutv'] == 7.0)                                        # nothing launched


@pytest.mark.parametrize('V,d', [(63, 64), (1001, 128)])
def test_direct_target_ranks(V, d):
    """The device's own answer where the host check is bypassed: a target outside its row's pool (or
    in a row whose pool index is no pool) gets rank -1 and value 0 and is counted nowhere."""
    c = ctx_of(V, d)
    rec, dev = c.rec, c.rec.dev
    cubes = [c.cubes[r] for r in (2, 3, 4, 8)]
    rows = [2, 3, 4, 8]
    pool_of_row = [0, 0, 1, -1]                                     # 1 == n_pools: no pool of the table
    member = c.member['every_other']
    rng = np.random.default_rng(V)
    targets = [rng.permutation(np.flatnonzero(~c.in_cube[r]))[:30] for r in rows]
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    tgt_ptr = np.zeros(5, np.int32)
    tgt_ptr[1:] = np.cumsum([len(t) for t in targets])
    tgt = np.concatenate(targets).astype(np.int32)
    cutoffs = (1, 5, 50)

    def run(null_pools=False, ws_shift=0):
        rp, ix, tp, tg = (torch.from_numpy(a).to(dev) for a in (row_ptr, idx, tgt_ptr, tgt))
        cut = torch.tensor(cutoffs, device=dev, dtype=torch.int32)
        por = torch.tensor(pool_of_row, device=dev, dtype=torch.int32)
        table = torch.from_numpy(c.pools['every_other'].words.view(np.int32).reshape(1, -1)).to(dev)
        ws = torch.full((int(L.lib().cc_recommend_batch_target_ranks_pool_ws_size(V, d, 4, max_n)) // 4 + 64,), -1,
                        device=dev, dtype=torch.int32)
        ranks = torch.full((len(tgt),), 77, device=dev, dtype=torch.int32)
        vals = torch.full((len(tgt),), 7.0, device=dev)
        hits = torch.zeros(5, device=dev, dtype=torch.int64)
        cutv = torch.full((len(idx),), 7.0, device=dev)
        rc = L.lib().cc_recommend_batch_target_ranks_pool_fp32(
            L.ptr(rec.params), V, d, 4, L.ptr(rp), L.ptr(ix), max_n, L.ptr(tp), L.ptr(tg),
            L.ptr(cut), 3, L.C.c_void_p(ws.data_ptr() + ws_shift),
            L.ptr(ranks), L.ptr(vals), L.ptr(hits), L.ptr(cutv), None,
            None if null_pools else L.ptr(table), 1, L.ptr(por), L.stream_ptr())
        torch.cuda.synchronize()
        return rc, ranks.cpu().numpy(), vals.cpu().numpy(), hits.cpu().numpy()

    rc, ranks, vals, hits = run()
    assert rc == 0
    valid = []
    for i, r in enumerate(rows):
        got_r, got_v = ranks[tgt_ptr[i]:tgt_ptr[i + 1]], vals[tgt_ptr[i]:tgt_ptr[i + 1]]
        name = {0: 'every_other', 1: 'empty', -1: None}[pool_of_row[i]]
        cand = c.cand(r, name)
        pos = np.full(V, -1, np.int64)
        pos[cand] = np.arange(len(cand))
        assert np.array_equal(got_r, pos[targets[i]])
        assert np.array_equal(got_v, np.where(pos[targets[i]] >= 0, c.p[r][targets[i]], np.float32(0)))
        valid.append(got_r[got_r >= 0])
    assert np.any(ranks[:tgt_ptr[2]] == -1) and np.any(ranks[:tgt_ptr[2]] >= 0)   # both kinds were there
    assert np.all(ranks[tgt_ptr[2]:tgt_ptr[3]] == -1) and np.all(ranks[tgt_ptr[3]:] >= 0)
    allv = np.concatenate(valid)
    assert hits.tolist() == [np.count_nonzero(allv < K) for K in cutoffs] + [
        len(allv), sum(1 for v in valid if len(v) and v.min() < 1)]
    for kw, word in ((dict(null_pools=True), b'pools is null'), (dict(ws_shift=4), b'aligned')):
        rc, ranks, vals, hits = run(**kw)
        assert rc == -1 and word in L.lib().cc_last_error_string()
        assert np.all(ranks == 77) and np.all(vals == 7.0) and not hits.any()
