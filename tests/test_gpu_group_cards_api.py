"""The archetype card profiles through the Python surface on the GPU: group_cards at several span
sizes, CubeCorpus.group_cards from the resident lists, CubeClusters.signature_cards over a small
planted corpus and api.archetype_cards, every integer equal to the reference
(tests/group_cards_ref.py), and the error cases."""
import numpy as np
import pytest

from tests import cube_cluster_ref as CR
from tests import group_cards_ref as R
from tests.test_gpu_cube_index import C, V, World

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def world():
    return World()


def reference(cubes, labels, V_, G, kind, min_count, m):
    lists = [np.unique(np.asarray(c, np.int64)) for c in cubes]
    count, size, total = R.counts(*R.csr(lists), labels, V_, G)
    return (count, size, total) + R.top(count, size, total, kind, min_count, m)


def same(res, want, counts=False):
    count, size, total, cards, ccnt, found = want
    ok = res.cards.dtype == np.int32 and res.card_count.dtype == np.uint32 and res.found.dtype == np.int32 \
        and np.array_equal(res.cards, cards) and np.array_equal(res.card_count, ccnt) \
        and np.array_equal(res.found, found) and np.array_equal(res.sizes, size) and np.array_equal(res.totals, total) \
        and res.N == int(size.sum())
    if counts:
        ok = ok and res.counts.dtype == np.uint32 and np.array_equal(res.counts, count)
    return ok and (counts or res.counts is None)


def labels_of(n, G, seed):
    lab = np.random.default_rng(seed).integers(-1, G, n).astype(np.int32)
    lab[lab == 3] = -1                            # an empty group
    return lab


def test_group_cards_whatever_the_span(world):
    from cubecobrarecommender_amd.groupcards import group_cards
    G = 7
    lab = labels_of(C, G, 1)
    for kind, min_count, m in (('lift', 1, 12), ('rate', 3, 5), ('avoid', 2, 40)):
        want = reference(world.cubes, lab, V, G, kind, min_count, m)
        for rows in (64, 1000, 65536):
            got = group_cards(world.cubes, lab, V, m, kind=kind, min_count=min_count, G=G, counts=True,
                              rows_per_launch=rows)
            assert same(got, want, counts=True), (kind, rows)
    got = group_cards(world.cubes, lab, V, 12)    # G from the labels, no counts
    assert got.G == 7 and same(got, reference(world.cubes, lab, V, 7, 'lift', 1, 12))
    rate = got.card_count[0, 0] / got.sizes[0]
    assert got.rate[0, 0] == rate and got.lift[0, 0] == rate - got.totals[got.cards[0, 0]] / got.N
    held = world.cubes[5]
    miss = got.missing(int(lab[5]) if lab[5] >= 0 else 0, held, 4)
    assert len(miss) <= 4 and not np.isin(miss, held).any()
    none = group_cards([], [], V, 3, G=2)         # no cubes: zero tables
    assert none.N == 0 and np.all(none.found == 0) and np.all(none.totals == 0) and np.all(none.cards == -1)


def test_corpus_group_cards_equals_group_cards(world):
    from cubecobrarecommender_amd.groupcards import group_cards
    corpus = world.model.cube_corpus(world.cubes)
    G = 5
    lab = labels_of(C, G, 2)
    for kind in R.KINDS:
        want = group_cards(world.cubes, lab, V, 9, kind=kind, G=G, counts=True)
        assert same(want, reference(world.cubes, lab, V, G, kind, 1, 9), counts=True)
        for rows in (100, 1 << 20):
            got = corpus.group_cards(lab, 9, kind=kind, G=G, counts=True, rows_per_launch=rows)
            for f in ('cards', 'card_count', 'found', 'sizes', 'totals', 'counts', 'rate', 'base', 'lift'):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (kind, rows, f)
    with pytest.raises(ValueError, match='labels for'):
        corpus.group_cards(lab[:-1], 9)
    with pytest.raises(ValueError, match='label 5'):
        corpus.group_cards(np.full(C, 5), 9, G=5)


def test_signature_cards_of_a_planted_corpus():
    """About 1,000 cubes around 5 planted centres, each centre with a block of 100 of the 500 cards
    its cubes mostly draw from: the clustering finds the centres, and every archetype's signature
    cards come from its block."""
    from cubecobrarecommender_amd import api
    from cubecobrarecommender_amd.cubesim import CubeIndex
    N, V_, k = 1000, 500, 5
    e, _ = CR.make_emb('planted', N, 64, seed=4, centres=k, copies=1)
    rng = np.random.default_rng(9)
    cubes = []
    for i in range(N):
        own = rng.choice(100, 30, replace=False) + 100 * (i % k)
        cubes.append(np.concatenate([own, rng.choice(V_, 10, replace=False)]))      # duplicates allowed
    res = CubeIndex.from_latents(e).cluster(k, init=[0, 1, 2, 3, 4])      # one cube of every centre
    assert sorted(res.sizes.tolist()) == [N // k] * k
    for kind, min_count in (('lift', 1), ('rate', 1), ('avoid', 5)):
        got = res.signature_cards(cubes, 20, kind=kind, min_count=min_count)
        assert same(got, reference(cubes, res.labels, V_, k, kind, min_count, 20)), kind
        for g in range(k):
            centre = int(np.flatnonzero(res.labels == g)[0]) % k
            block = got.cards[g] // 100 == centre
            assert block.all() if kind != 'avoid' else not block.any(), (kind, g)
    rows = api.archetype_cards(res, cubes, 20, int_to_card={i: f'card{i}' for i in range(V_)})
    got = res.signature_cards(cubes, 20)
    assert [r['id'] for r in rows] == list(range(k)) and [r['size'] for r in rows] == res.sizes.tolist()
    assert rows[2]['cards'][0] == (f'card{got.cards[2, 0]}', got.rate[2, 0], got.lift[2, 0])
    assert len(rows[0]['cards']) == 20 and rows[0]['cards'][0][2] > 0.2
    with pytest.raises(ValueError, match='cubes for a clustering'):
        res.signature_cards(cubes[:-1], 20)


def test_signature_cards_from_a_corpus(world):
    res = world.index.cluster(6, seed=3)
    corpus = world.model.cube_corpus(world.cubes)
    a, b = res.signature_cards(corpus, 10), res.signature_cards(world.cubes, 10)
    assert same(a, reference(world.cubes, res.labels, V, 6, 'lift', 1, 10))
    assert np.array_equal(a.cards, b.cards) and np.array_equal(a.card_count, b.card_count)
    with pytest.raises(ValueError, match='cubes for a clustering'):
        res.signature_cards(world.model.cube_corpus(world.cubes[:50]), 10)


def test_error_cases_launch_nothing(world):
    from cubecobrarecommender_amd.groupcards import group_cards
    lab = labels_of(C, 4, 3)
    for kw, what in ((dict(labels=lab[:-1]), 'labels for'), (dict(m=0), 'm = 0'), (dict(m=1025), 'm = 1025'),
                     (dict(kind='best'), 'kind'), (dict(G=2), 'label'), (dict(G=1025), 'G = 1025'),
                     (dict(V=V - 200), 'outside'), (dict(V=(1 << 18) + 1), 'V ='), (dict(min_count=-1), 'min_count')):
        with pytest.raises(ValueError, match=what):
            group_cards(**{**dict(cubes=world.cubes, labels=lab, V=V, m=5), **kw})
