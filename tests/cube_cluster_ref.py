"""Reference of the cube archetypes (cc_cube_cluster, cc_cube_assign) for the tests:
the pinned arithmetic in numpy, every intermediate cast to float32 (host only).

  rows     n = the put's normalisation of the raw embeddings: ss = sum e[t]^2 in index order,
           inv = 1 / sqrt(max(ss, 1e-12)), n[t] = e[t] * inv
  assign   dist(i, j) = -(sum_t n_i[t] * c_j[t]) in ascending t from +0, multiply and add separately
           rounded; label = the lowest j of the smallest distance, dist = that distance
  update   P[b][j] = sum of n_i over block b's cubes with label j in ascending i; S[j] = sum of
           P[b][j] in ascending b; S[j] normalised like a put row, a cluster without members keeps
           its centroid
  loop     as include/ccrec.h states it
The id block B is the library's constant (cc_cube_cluster_block())."""
import numpy as np

from tests import cube_sim_ref

EPS = np.float32(1e-12)
KINDS = cube_sim_ref.KINDS + ('planted',)


def block():
    from cubecobrarecommender_amd import _lib as L
    return int(L.lib().cc_cube_cluster_block())


def make_emb(kind, N, K, seed, centres=8, copies=4):
    """cube_sim_ref.make_emb's kinds, and 'planted': `centres` cluster centres, every cube one of
    them (cube i: centre i % centres) plus 0.1-sigma noise, and the corpus repeats its first
    N // copies cubes (row i is row i % (N // copies)).  Start ids that hit copies of one cube give
    equal centroids: the higher one stays empty wherever the lower one keeps the copies, so this
    kind leaves clusters empty.  (embeddings [N, K], the rows worth asking about)."""
    if kind != 'planted':
        return cube_sim_ref.make_emb(kind, N, K, seed)
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((centres, K)).astype(np.float32)
    e = (mu[np.arange(N) % centres] + np.float32(0.1) * rng.standard_normal((N, K)).astype(np.float32))
    distinct = N // copies
    if distinct >= centres:
        e = e[np.arange(N) % distinct]
    return e.astype(np.float32), []


def normalise(e):
    """The index rows of raw embeddings e [N, K] (cc_cube_index_put)."""
    e = np.asarray(e, np.float32).reshape(len(e), -1)
    ss = np.zeros(len(e), np.float32)
    for t in range(e.shape[1]):
        ss = (ss + (e[:, t] * e[:, t]).astype(np.float32)).astype(np.float32)
    inv = (np.float32(1) / np.sqrt(np.maximum(ss, EPS))).astype(np.float32)
    return (e * inv[:, None]).astype(np.float32)


def all_dists(n, c):
    """dist [R, k] of rows n [R, K] to centroids c [k, K]."""
    n, c = np.asarray(n, np.float32), np.asarray(c, np.float32)
    dot = np.zeros((len(n), len(c)), np.float32)
    for t in range(n.shape[1]):
        dot = (dot + (n[:, t:t + 1] * c[None, :, t]).astype(np.float32)).astype(np.float32)
    return (-dot).astype(np.float32)


def assign(n, c):
    """(label int32 [R], dist float32 [R]): argmin takes the first of equal distances, and no
    distance is +0 (a dot starts from +0 and is never -0), so -0 and +0 never meet."""
    d = all_dists(n, c)
    label = np.argmin(d, axis=1).astype(np.int32)
    return label, d[np.arange(len(d)), label].astype(np.float32)


def update(n, label, c, B):
    """The centroids after one update of c with the labels of rows n."""
    n, c = np.asarray(n, np.float32), np.asarray(c, np.float32)
    k, K = c.shape
    N, blocks = len(n), -(-len(n) // B)
    size = np.bincount(label, minlength=k)
    # a cube's turn inside its (block, label) group: the groups' sums advance together, one member
    # each per step, which is every group's own ascending-id order
    group = (np.arange(N) // B) * k + label
    order = np.argsort(group, kind='stable')
    start = np.flatnonzero(np.r_[True, group[order][1:] != group[order][:-1]])
    turn = np.empty(N, np.int64)
    turn[order] = np.arange(N) - np.repeat(start, np.diff(np.r_[start, N]))
    P = np.zeros((blocks * k, K), np.float32)
    for step in range(int(turn.max()) + 1 if N else 0):
        rows = np.flatnonzero(turn == step)
        P[group[rows]] = (P[group[rows]] + n[rows]).astype(np.float32)
    S = np.zeros((k, K), np.float32)
    for b in range(blocks):
        S = (S + P[b * k:(b + 1) * k]).astype(np.float32)
    out = c.copy()
    live = size > 0
    out[live] = normalise(S[live])
    return out


def cluster(n, init_ids, max_iter, B=None):
    """cc_cube_cluster on index rows n [N, K]: dict(label, dist, centroids, sizes, changed, n_iter,
    converged)."""
    B = B or block()
    n = np.asarray(n, np.float32)
    N = len(n)
    init_ids = np.asarray(init_ids, np.int64)
    assert init_ids.min() >= 0 and init_ids.max() < N
    c = n[init_ids].copy()
    prev = np.full(N, -1, np.int32)
    changed = np.full(max_iter + 1, -1, np.int32)
    n_iter = max_iter
    for t in range(max_iter + 1):
        label, dist = assign(n, c)
        changed[t] = int((label != prev).sum())
        prev = label
        if t == max_iter:
            break
        if changed[t] == 0:
            n_iter = t
            break
        c = update(n, label, c, B)
    return dict(label=label, dist=dist, centroids=c, sizes=np.bincount(label, minlength=len(c)).astype(np.int32),
                changed=changed, n_iter=n_iter, converged=bool(changed[n_iter] == 0))


def objective(dist):
    """The mean cosine similarity of the cubes to their centroids, in float64."""
    return float(-np.asarray(dist, np.float64).mean()) if len(dist) else 0.0


def init_ids(N, k, seed):
    """k distinct member ids: CubeIndex.cluster's draw for restart 0 of `seed`."""
    return np.random.default_rng(seed).choice(N, k, replace=False).astype(np.int32)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)
