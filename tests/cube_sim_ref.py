"""Reference of the cube-neighbour search for the tests (host only).  The distances are
oracle.similarity_ref.cosine_dists, unchanged; the expected row of a query is: its distances to all
N cubes, the skipped cube dropped, numpy's stable argsort, the first k, then -1 / 0.f."""
import numpy as np

from oracle import similarity_ref

KINDS = ('relu', 'signed', 'zero-rows', 'dups', 'allzero', 'tiny')


def make_emb(kind, V, K, seed):
    """tests/test_gpu_similarity_batch.py's make_emb, restated: finite embeddings of one kind, and
    the rows worth asking about."""
    rng = np.random.default_rng(seed)
    e = np.maximum(rng.standard_normal((V, K)).astype(np.float32), 0)
    special = []
    if kind == 'signed':
        e = (rng.standard_normal((V, K)) * np.exp2(rng.uniform(-8, 8, size=(V, K)))).astype(np.float32)
    elif kind == 'zero-rows':
        special = sorted({z for z in (1, 2, V - 1) if 0 <= z < V})
        e[special] = 0
    elif kind == 'dups' and V > 12:
        for a, b in ((10, 11), (10, V - 2), (3, 4)):
            e[b] = e[a]
        special = [10, 11, V - 2, 3, 4]
    elif kind == 'allzero':
        e[:] = 0
    elif kind == 'tiny':
        row = min(5, V - 1)
        e[row] = np.float32(1e-8) * (1 + rng.random(K)).astype(np.float32)       # ss <= 4 K 1e-16 < 1e-12
        assert float((e[row].astype(np.float64) ** 2).sum()) < 1e-12
        special = [row]
    assert np.all(np.isfinite(e))
    return e, special


def make_queries(V, special, Q, seed):
    """Q ids: 0 and V - 1, the special rows, the same id twice, then random ones."""
    rng = np.random.default_rng(seed + 1)
    head = [0, V - 1] + list(special) + [V // 2, V // 2]
    return np.array(head + rng.integers(0, V, size=max(0, Q)).tolist(), np.int32)[:Q]


def member_dists(emb, q):
    """Distances of member cube q to every cube of emb [N, K]."""
    return similarity_ref.cosine_dists(emb, int(q))


def fresh_dists(emb, z):
    """Distances of the raw embedding z [K] to every cube of emb: z as one more row of the matrix
    (every row's arithmetic is its own), the distance to itself dropped."""
    ext = np.concatenate([np.asarray(emb, np.float32), np.asarray(z, np.float32)[None, :]])
    return similarity_ref.cosine_dists(ext, len(emb))[:len(emb)]


def expected_row(d, k, skip=-1, order=None):
    """(indices int32 [k], dists float32 [k]) for the distances d [N] to all cubes; order: d's
    stable argsort where the caller has kept it."""
    if order is None:
        order = np.argsort(d, kind='stable')
    if 0 <= skip < len(d):
        order = order[order != skip]
    order = order[:k]
    idx = np.full(k, -1, np.int32)
    dist = np.zeros(k, np.float32)
    idx[:len(order)] = order
    dist[:len(order)] = d[order]
    return idx, dist


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)
