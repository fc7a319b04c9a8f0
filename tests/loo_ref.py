"""Leave-one-out reference: oracle.infer_ref.recommend_probs on the sorted distinct ids without
the one at position j, read at the wanted cards.  The output kernel's columns are sliced before the
last dense32: a column's dot product does not depend on the others, so the values are the bits
of the full row's."""
import numpy as np

from oracle import infer_ref
from oracle.detmath import det_sigmoid32


def h3_of(P, ids):
    """The decoder's last hidden layer of the cube `ids` (any order, duplicates collapse)."""
    h = infer_ref.encode32(P, ids)
    for nm in infer_ref.TOWER[3:]:
        h = infer_ref.dense32(h, P[nm + '/kernel'], P[nm + '/bias'])
    return h


def probs_at(P, ids, cards):
    """recommend_probs(P, ids)[cards] without the other columns."""
    cards = np.asarray(cards, np.int64).reshape(-1)
    if not len(cards):
        return np.zeros(0, np.float32)
    Wo, bo = P['decoder/reconstruct/kernel'], P['decoder/reconstruct/bias']
    return det_sigmoid32(infer_ref.dense32(h3_of(P, ids), Wo[:, cards], bo[cards], relu=False))


def without(ids, j):
    """The sorted distinct ids of `ids` without the one at sorted position j."""
    u = np.unique(np.asarray(ids, np.int64))
    return np.delete(u, j)


def loo_self(P, cube):
    """(loo_vals, cut_vals) of `cube` in its input order: p(c | cube without c) and p(c | cube)."""
    cube = np.asarray(cube, np.int64).reshape(-1)
    u = np.unique(cube)
    loo = np.array([probs_at(P, without(u, j), [u[j]])[0] for j in range(len(u))], np.float32).reshape(-1)
    cut = probs_at(P, u, u)
    at = np.searchsorted(u, cube)
    return loo[at], cut[at]


def loo_targets(P, cube, targets):
    """(base [T], without [m, T]) of `cube` in its input order at the cards `targets`."""
    cube = np.asarray(cube, np.int64).reshape(-1)
    targets = np.asarray(targets, np.int64).reshape(-1)
    u = np.unique(cube)
    rows = np.zeros((len(u), len(targets)), np.float32)
    for j in range(len(u)):
        rows[j] = probs_at(P, without(u, j), targets)
    return probs_at(P, u, targets), rows[np.searchsorted(u, cube)]
