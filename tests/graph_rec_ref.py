"""The co-occurrence baseline's pinned definition in numpy (test infra; the reference of
tests/test_graph_rec_host.py and tests/test_gpu_graph_rec.py).

For a cube S (sorted distinct ids) over an f64 matrix M [V][ld >= V]:

    score[j] = fold over i in S ascending of  acc = acc + (i == j ? +0.0 : M[i][j]),  acc from +0.0

in f64, every add rounded.  Additions: the cards outside S in descending score, equal scores
higher index first (argsort(kind='stable')[::-1]).  Cuts: the cards of S in ascending score, equal
scores lower index first (argsort(kind='stable')).  Comparisons are numeric: -0.0 equals +0.0.
"""
import numpy as np


def cube_of(cards):
    """Sorted distinct ids (the CSR row) of a card list."""
    return np.unique(np.asarray(cards, np.int64).reshape(-1))


def scores(M, cube):
    """score[0 .. V) of the cube: an explicit loop over its ids in ascending order, one rounded
    elementwise f64 add per id."""
    V = M.shape[0]
    acc = np.zeros(V, np.float64)
    for i in cube_of(cube):
        row = np.array(M[i, :V], np.float64)
        row[i] = 0.0
        acc = acc + row
    return acc


def additions(score, cube, amount):
    """(cards int32, values f64): the first min(max(amount, 1), V - n) of the ranking."""
    V = len(score)
    missing = np.setdiff1d(np.arange(V), cube_of(cube))
    order = missing[np.argsort(score[missing], kind='stable')[::-1]]
    want = min(max(int(amount), 1), len(missing))
    return order[:want].astype(np.int32), score[order[:want]]


def cuts(score, cube):
    """(cards int32, values f64) of the cube in cut order."""
    ids = cube_of(cube)
    order = ids[np.argsort(score[ids], kind='stable')]
    return order.astype(np.int32), score[order]


def positions(score, cube):
    """pos[c] = position of card c in the full ranking of the additions, -1 for a cube card."""
    V = len(score)
    order, _ = additions(score, cube, V)
    pos = np.full(V, -1, np.int64)
    pos[order] = np.arange(len(order))
    return pos


def target_ranks(score, cube, targets):
    """(ranks int32, values f64) of a target list that may hold invalid ids: -1 / 0 for an id
    outside [0, V) or inside the cube."""
    V = len(score)
    pos = positions(score, cube)
    t = np.asarray(targets, np.int64).reshape(-1)
    ok = (t >= 0) & (t < V)
    ranks = np.full(len(t), -1, np.int32)
    ranks[ok] = pos[t[ok]]
    vals = np.zeros(len(t), np.float64)
    good = ranks >= 0
    vals[good] = score[t[good]]
    return ranks, vals


class HostGraphRecommender:
    """GraphRecommender's interface over the functions above: what the CPU tests put in its
    place.  Records the calls it gets."""

    def __init__(self, adj, device='cuda'):
        self.adj = np.asarray(adj)
        self.V = self.adj.shape[0]
        self.calls = []

    def recommend_many(self, cubes, amount, want_scores=False, rows_per_launch=512):
        self.calls.append(('recommend_many', [list(map(int, c)) for c in cubes], int(amount), want_scores))
        out = []
        for c in cubes:
            s = scores(self.adj, c)
            a, av = additions(s, c, amount)
            k, kv = cuts(s, c)
            o = {'additions': a, 'add_vals': av, 'cuts': k, 'cut_vals': kv}
            if want_scores:
                o['scores'] = s
            out.append(o)
        return out
