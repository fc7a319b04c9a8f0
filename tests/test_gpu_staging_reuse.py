"""The kept pinned staging of the two full-ranking paths across launches and calls: many launches
through both staging sets, then a call that takes smaller views of the kept buffers and leaves some
keys unused, then the first call again.  Every result equals, bit for bit, the same request on a
fresh object in a single launch, and the arrays of an earlier call survive the later ones (a result
that were a view of the staging would not)."""
import copy

import numpy as np
import pytest

from cubecobrarecommender_amd.graphrec import GraphRecommender
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import Recommender
from oracle import model_ref
from tests.test_gpu_graph_rec import edge_cubes, matrix_of
from tests.test_gpu_recommend_rank import ALL, limit, mixed_batch

pytestmark = pytest.mark.gpu

V, D = 63, 64               # the smallest model and graph of the rank tests


def assert_same_bits(got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w), r
        for k in w:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (r, k)
            word = f'u{w[k].itemsize}'                     # integers as they are, floats by their bits
            assert np.array_equal(np.ascontiguousarray(g[k]).view(word), np.ascontiguousarray(w[k]).view(word)), (r, k)


def check_sequence(make, call_a, call_b):
    """call A (five launches of at most two rows), call B (one launch, fewer rows and outputs),
    call A again on one object; the expected values from a fresh object and a single launch each."""
    want_a, want_b = call_a(make(), 512), call_b(make(), 512)
    rec = make()
    first = call_a(rec, 2)
    held = copy.deepcopy(first)
    assert_same_bits(first, want_a)
    b = call_b(rec, 512)
    assert_same_bits(b, want_b)
    again = call_a(rec, 2)
    assert_same_bits(again, want_a)
    assert_same_bits(first, held)                          # untouched by the two later calls
    assert_same_bits(b, want_b)
    return rec


def test_recommender_full_ranking():
    assert ALL > limit()                                   # the full-ranking path
    P = model_ref.init_params(V, D, seed=V + D, bias_std=0.01)
    params = Layout(V, D).pack(P)
    cubes = mixed_batch(V)
    assert len(cubes) == 11
    rec = check_sequence(
        lambda: Recommender(params, V, D),
        lambda rec, rows: rec.recommend_many(cubes[:9], ALL, want_probs=True, rows_per_launch=rows),
        lambda rec, rows: rec.recommend_many(cubes[8:], ALL, rows_per_launch=rows))
    assert set(rec._rank_pins.bufs) == {(turn, i) for turn in (0, 1) for i in range(3)}


def test_graph_rank_many():
    M = matrix_of(V, 'wild')
    cubes = edge_cubes(V, rows=12)
    rec = check_sequence(
        lambda: GraphRecommender(M),
        lambda rec, rows: rec.rank_many(cubes[:9], want_vals=True, want_scores=True, rows_per_launch=rows),
        lambda rec, rows: rec.rank_many(cubes[9:], want_vals=False, want_scores=False, rows_per_launch=rows))
    assert set(rec._rank_pins.bufs) == {(turn, name) for turn in (0, 1)
                                        for name in ('ints', 'vals', 'cutv', 'scores')}
