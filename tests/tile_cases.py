"""The shapes at which the shared dot-product tile (csrc/dottile.hpp) can go wrong, with the model,
the cubes and the oracle's probabilities that the GPU test files share at them (computed once, never
changed).  Every case is (V, d, rows):
  V = 299   no multiple of the tile's 64 columns, nor of a lane's 4
  d = 64    one pinned chunk of k in two LDS stages;  d = 192: an odd number of chunks
  rows      one more than a row tile of 32 / 64 / 128, the heights the entries dispatch
"""
import numpy as np

from oracle import infer_ref, model_ref

TILE_CASES = [(299, 64, 33), (299, 192, 65), (299, 192, 129)]
MAX_ROWS = max(r for _, _, r in TILE_CASES)
_params, _recs, _cubes, _probs = {}, {}, {}, {}


def params(V, d):
    if (V, d) not in _params:
        _params[(V, d)] = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
    return _params[(V, d)]


def recommender(V, d):
    from cubecobrarecommender_amd.layout import Layout
    from cubecobrarecommender_amd.recommender import Recommender
    if (V, d) not in _recs:
        _recs[(V, d)] = Recommender(Layout(V, d).pack(params(V, d)), V, d)
    return _recs[(V, d)]


def cubes(V, rows):
    """`rows` cubes of 0..60 distinct cards; row 0 is empty, row 1 holds one card."""
    if V not in _cubes:
        rng = np.random.default_rng(V)
        sizes = [0, 1] + [int(n) for n in rng.integers(2, 61, MAX_ROWS - 2)]
        _cubes[V] = [rng.choice(V, n, replace=False) for n in sizes]
    return _cubes[V][:rows]


def probs(V, d, rows):
    """infer_ref.recommend_probs of every cube."""
    if (V, d) not in _probs:
        _probs[(V, d)] = [infer_ref.recommend_probs(params(V, d), c) for c in cubes(V, MAX_ROWS)]
    return _probs[(V, d)][:rows]
