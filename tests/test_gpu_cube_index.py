"""CubeIndex on the GPU through the Python surface: a small model, about 700 synthetic cubes (some
identical, one empty), every result against encode_lists + the oracle ranking
(tests/cube_sim_ref.py), bit for bit on uint32 views."""
import os
import sys

import numpy as np
import pytest

from tests import cube_sim_ref as R
from tests.cube_sim_ref import u32

pytestmark = pytest.mark.gpu

V, D, C, K = 300, 64, 700, 12
TWINS = ((20, 500), (3, 699), (64, 65))       # identical cubes, in and across 64-cube chunks
EMPTY = 17


def make_cubes(seed=5):
    rng = np.random.default_rng(seed)
    cubes = [rng.choice(V, size=int(rng.integers(5, 60)), replace=False).astype(np.int64) for _ in range(C)]
    for a, b in TWINS:
        cubes[b] = cubes[a][::-1].copy()      # the same cards in another order
    cubes[EMPTY] = np.zeros(0, np.int64)
    return cubes


class World:
    def __init__(self):
        from cubecobrarecommender_amd.model import CC_Recommender
        self.model = CC_Recommender(V, d=D, seed=11)
        self.cubes = make_cubes()
        self.index = self.model.cube_index(self.cubes)
        self.z = self.model.recommender().encode_lists(self.cubes).cpu().numpy()
        self._d = {}

    def expected(self, ids, k, exclude_self):
        rows = []
        for q in ids:
            q = int(q)
            if q not in self._d:
                d = R.member_dists(self.z, q)
                self._d[q] = (d, np.argsort(d, kind='stable'))
            d, order = self._d[q]
            rows.append(R.expected_row(d, k, q if exclude_self else -1, order=order))
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@pytest.fixture(scope='module')
def world():
    return World()


def same(got, want):
    return got[0].dtype == np.int32 and got[1].dtype == np.float32 and np.array_equal(got[0], want[0]) \
        and np.array_equal(u32(got[1]), u32(want[1]))


QUERIES = np.array([0, C - 1, EMPTY, 20, 500, 3, 699, 64, 65, 350, 350] + list(range(100, 160)), np.int64)


def test_rows_equal_the_encoder_and_the_oracle(world):
    assert len(world.index) == C and world.index.capacity == C
    for exclude in (True, False):
        got = world.index.neighbours(QUERIES, K, exclude_self=exclude)
        assert got[0].shape == (len(QUERIES), K)
        assert same(got, world.expected(QUERIES, K, exclude)), exclude
    n = C - 1                                                   # k above the corpus: every other cube
    got = world.index.neighbours(QUERIES[:4], 1000)
    assert got[0].shape == (4, n) and same(got, world.expected(QUERIES[:4], n, True))
    got = world.index.neighbours(QUERIES[:4], 1000, exclude_self=False)
    assert got[0].shape == (4, C) and same(got, world.expected(QUERIES[:4], C, False))
    for k in (0, -3):
        gi, gd = world.index.neighbours(QUERIES, k)
        assert gi.shape == gd.shape == (len(QUERIES), 0)


def test_identical_cubes_are_each_others_first_neighbour(world):
    a = np.array([t[0] for t in TWINS]), np.array([t[1] for t in TWINS])
    ids = np.concatenate(a)
    gi, gd = world.index.neighbours(ids, 3)
    si, sd = world.index.neighbours(ids, 3, exclude_self=False)
    assert gi[:, 0].tolist() == np.concatenate(a[::-1]).tolist()
    # with itself in, the pair leads in id order, both at the self distance's bits
    assert np.array_equal(si[:, :2], np.tile(np.stack(a, 1), (2, 1)))
    assert np.array_equal(u32(sd[:, 0]), u32(sd[:, 1])) and np.array_equal(u32(gd[:, 0]), u32(sd[:, 0]))


def test_fresh_against_member(world):
    ids = QUERIES[:20]
    want = world.index.neighbours(ids, K, exclude_self=False)
    got = world.index.neighbours_of([world.cubes[int(j)] for j in ids], K)
    assert same(got, want)
    from cubecobrarecommender_amd import api
    rows = api.similar_cubes(world.index, world.cubes[20], 5)
    assert [r[0] for r in rows] == [1, 2, 3, 4, 5] and [r[1] for r in rows] == want[0][3, :5].tolist()
    assert u32(np.array([r[2] for r in rows], np.float32)).tolist() == u32(want[1][3, :5]).tolist()
    names = [f'cube {i}' for i in range(C)]
    assert [r[1] for r in api.similar_cubes(world.index, world.cubes[20], 5, names)] == \
        [names[j] for j in want[0][3, :5]]
    stranger = [1, 2, 3, 250, 299, 299]                         # no member; duplicates count once
    z = world.model.recommender().encode_lists([stranger]).cpu().numpy()[0]
    want_row = R.expected_row(R.fresh_dists(world.z, z), K)
    assert same(world.index.neighbours_of([stranger], K), [w[None] for w in want_row])


def test_results_do_not_depend_on_the_batching(world):
    base = world.index.neighbours(QUERIES, K)
    fresh = [world.cubes[int(j)] for j in QUERIES]
    base_f = world.index.neighbours_of(fresh, K)
    for rows in (1, 3, 512):
        for chunk in (64, 0):
            assert same(world.index.neighbours(QUERIES, K, rows_per_launch=rows, chunk=chunk), base), (rows, chunk)
            gi, gd = world.index.neighbours(QUERIES[::-1].copy(), K, rows_per_launch=rows, chunk=chunk)
            assert same((gi[::-1], gd[::-1]), base), (rows, chunk)
            assert same(world.index.neighbours_of(fresh, K, rows_per_launch=rows, chunk=chunk), base_f), (rows, chunk)


def test_add_in_pieces_equals_construction(world):
    from cubecobrarecommender_amd.cubesim import CubeIndex
    grown = CubeIndex(world.model, world.cubes[:250], capacity=C + 5, rows_per_launch=100)
    assert len(grown) == 250
    assert grown.add(world.cubes[250:251]) == range(250, 251)
    assert grown.add(world.cubes[251:], rows_per_launch=128) == range(251, C)
    assert grown.add([]) == range(C, C) and len(grown) == C
    assert same(grown.neighbours(QUERIES, K), world.index.neighbours(QUERIES, K))
    with pytest.raises(ValueError, match='capacity'):
        grown.add(world.cubes[:6])
    assert len(grown) == C
    assert grown.add(world.cubes[:5]) == range(C, C + 5)        # exactly full
    with pytest.raises(ValueError, match='capacity'):
        grown.add(world.cubes[:1])
    with pytest.raises(ValueError, match='outside'):
        grown.neighbours([C + 5], K)
    rec = world.model.recommender()
    assert len(rec.cube_index(world.cubes[:10], capacity=20)) == 10


def test_table_and_cli(world, tmp_path, monkeypatch):
    ti, td = world.index.table(K, rows_per_launch=128)
    want = world.index.neighbours(np.arange(C), K)
    assert ti.shape == (C, K) and same((ti, td), want)
    assert same((ti[QUERIES], td[QUERIES]), world.expected(QUERIES, K, True))
    # the CLI on the same cubes: the model saved and loaded, the cubes through --synthetic
    dest = tmp_path / 'ml_files'
    world.model.save(str(dest / 'tiny'), save_format='tf')
    from cubecobrarecommender_amd import synthetic
    indptr = np.zeros(C + 1, np.int64)
    indptr[1:] = np.cumsum([len(c) for c in world.cubes])
    flat = np.concatenate(world.cubes).astype(np.int32)
    monkeypatch.setattr(synthetic, 'synthetic_cubes', lambda C_, V_, seed=0: (indptr, flat))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from scripts import similar_cubes as cli
    lines = []
    out = tmp_path / 'cubes.npz'
    cli.main(['tiny', str(K), '--out', str(out), '--synthetic', str(C), str(V), '--out-dir', str(dest)],
             print_fn=lambda *a: lines.append(' '.join(str(x) for x in a)))
    got = np.load(out)
    assert same((got['indices'], got['dists']), (ti, td))
    assert len(lines) == 1 and '\n' not in lines[0] and f'{C} cubes x {K}' in lines[0]
    lines.clear()
    cli.main(['tiny', '3', '--query', '20', '3', '--synthetic', str(C), str(V), '--out-dir', str(dest)],
             print_fn=lambda *a: lines.append(a))
    assert [(a[0], a[1], a[2]) for a in lines] == [(20, r + 1, int(ti[20, r])) for r in range(3)] + \
        [(3, r + 1, int(ti[3, r])) for r in range(3)]
