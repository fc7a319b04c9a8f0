"""Cube archetypes: deterministic spherical k-means over the member cubes of a
CubeIndex (cc_cube_cluster: all iterations queued on one stream, no host round trip between them)
and the nearest centroid of member or fresh cubes (cc_cube_assign).  Every bit of a result is fixed
by the index, k, the initial ids and max_iter."""
import numpy as np
import torch

from . import _lib as L
from .launches import mark, pipelined, row_spans, upload
from .recommender import check_card_ids

LATENT = 64   # cubesim.LATENT (this module is imported by cubesim)


def objective_of(dists):
    """The mean cosine similarity of cubes to their centroids, in float64 on the host."""
    return float(-np.asarray(dists, np.float64).mean()) if len(dists) else 0.0


def initial_ids(N, k, seed, restart=0):
    """The k distinct member ids restart `restart` of `seed` starts from."""
    return np.random.default_rng(int(seed) + restart).choice(N, k, replace=False).astype(np.int32)


def check_cluster_args(N, k, init, max_iter, n_init):
    """(k, init int32 [k] or None, max_iter, n_init), or ValueError: before any device call."""
    k, max_iter, n_init = int(k), int(max_iter), int(n_init)
    if k < 1:
        raise ValueError(f'k = {k} is below 1')
    if k > N:
        raise ValueError(f'k = {k} is above the {N} cubes of the index')
    cap = int(L.lib().cc_cube_cluster_max_k())
    if k > cap:
        raise ValueError(f'k = {k} is above cc_cube_cluster_max_k() = {cap}')
    if max_iter < 0:
        raise ValueError(f'max_iter = {max_iter} is negative')
    if n_init < 1:
        raise ValueError(f'n_init = {n_init} is below 1')
    if init is not None:
        init = np.asarray(init, np.int64).reshape(-1)
        if len(init) != k:
            raise ValueError(f'init holds {len(init)} ids, not k = {k}')
        bad = np.flatnonzero((init < 0) | (init >= N))
        if len(bad):
            raise ValueError(f'init {int(bad[0])}: cube id {int(init[bad[0]])} outside [0, {N})')
        init = init.astype(np.int32)
    return k, init, max_iter, n_init


class CubeClusters:
    """A clustering of the cubes [0, N) an index held when CubeIndex.cluster ran: a snapshot, cubes
    added later are unlabelled until predicted.
      labels int32 [N], dists float32 [N]   every cube's centroid and its cosine distance to it
      centroids float32 [k, K]              unit rows (host; `centroids_dev` is the device copy)
      sizes int32 [k]; n_iter; converged; changed int32 [max_iter + 1] (-1 behind n_iter)
      objective                             the mean cosine similarity, -dists.mean() in float64
      init                                  the ids it started from"""

    def __init__(self, index, init, labels, dists, centroids_dev, centroids, sizes, changed, n_iter):
        self.index, self.init = index, init
        self.labels, self.dists, self.sizes, self.changed = labels, dists, sizes, changed
        self.centroids_dev, self.centroids = centroids_dev, centroids
        self.k, self.N, self.n_iter = len(sizes), len(labels), int(n_iter)
        self.converged = bool(changed[self.n_iter] == 0)
        self.objective = objective_of(dists)

    def _assign(self, Q, qid, fresh, rows_per_launch):
        """cc_cube_assign in launches of up to rows_per_launch rows; qid int32 [Q] or None, fresh
        card-id arrays (encoded per launch) or None."""
        labels, dists = np.empty(Q, np.int32), np.empty(Q, np.float32)
        if Q == 0:
            return labels, dists
        index, dev, k = self.index, self.index.dev, self.k

        def launch(r0, r1, turn):
            Rc = r1 - r0
            ws = index._ws.get(L.lib().cc_cube_cluster_ws_size(0, LATENT, k, Rc), dev)
            q_d = upload(qid[r0:r1], dev) if qid is not None else None
            z_d = index._encode(fresh[r0:r1]) if fresh is not None else None
            lab = torch.empty(Rc, device=dev, dtype=torch.int32)
            dist = torch.empty(Rc, device=dev, dtype=torch.float32)
            L.call('cc_cube_assign', L.ptr(index._buf), index.capacity, N, LATENT, k, L.ptr(self.centroids_dev), Rc,
                   L.ptr(q_d), L.ptr(z_d), L.ptr(ws), L.ptr(lab), L.ptr(dist), L.stream_ptr())
            return (index._stage.fresh(lab), index._stage.fresh(dist)), mark()

        def collect(r0, r1, host):
            labels[r0:r1] = host[0].numpy()
            dists[r0:r1] = host[1].numpy()

        with index.lock:
            N = index.N
            last = pipelined(row_spans(Q, rows_per_launch), launch, collect)
            torch.cuda.current_stream().synchronize()   # the workspace is free for the next caller's stream
            del last                  # only now (launches.pipelined)
        return labels, dists

    def predict(self, ids, rows_per_launch=4096):
        """(labels int32 [Q], dists float32 [Q]) of member cubes of the index as it is now (cubes
        added since the clustering included); the same bits whatever rows_per_launch.  An id
        outside [0, len(index)) raises ValueError before anything is launched."""
        q = np.asarray(list(ids) if isinstance(ids, range) else ids, np.int64).reshape(-1)
        N = self.index.N
        bad = np.flatnonzero((q < 0) | (q >= N))
        if len(bad):
            raise ValueError(f'query {int(bad[0])}: cube id {int(q[bad[0]])} outside [0, {N})')
        return self._assign(len(q), q.astype(np.int32), None, rows_per_launch)

    def predict_cubes(self, cubes, rows_per_launch=4096):
        """`predict` for fresh cubes given as card-id lists, encoded on the device; a member cube
        asked this way gets the bits predict([j]) returns."""
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        check_card_ids(inputs, self.index.V)
        return self._assign(len(inputs), None, inputs, rows_per_launch)

    def members(self, c):
        """The ids of cluster c's cubes, ascending."""
        return np.flatnonzero(self.labels == self._cluster(c)).astype(np.int32)

    def representatives(self, c, m):
        """The up to m members of cluster c nearest its centroid, ordered by (dist, id)."""
        ids = self.members(c)
        return ids[np.argsort(self.dists[ids], kind='stable')[:max(0, int(m))]]

    def signature_cards(self, cubes_or_corpus, m, kind='lift', min_count=1):
        """What every archetype plays: groupcards.GroupCards of the clustered cubes
        under `labels`, m cards per cluster.  cubes_or_corpus: the N cubes of the clustering as
        card-id lists in id order, or an audience.CubeCorpus holding exactly them; any other count
        raises ValueError."""
        from . import groupcards
        if len(cubes_or_corpus) != self.N:
            raise ValueError(f'{len(cubes_or_corpus)} cubes for a clustering of {self.N}')
        if hasattr(cubes_or_corpus, 'group_cards'):
            return cubes_or_corpus.group_cards(self.labels, m, kind=kind, min_count=min_count, G=self.k)
        V = self.index.V      # an index of given latents knows no cards: the cubes' own range then
        if not V:
            V = max([int(np.max(c)) + 1 for c in cubes_or_corpus if len(c)], default=1)
        return groupcards.group_cards(cubes_or_corpus, self.labels, V, m, kind=kind, min_count=min_count, G=self.k,
                                      device=self.index.dev)

    def _cluster(self, c):
        c = int(c)
        if not 0 <= c < self.k:
            raise ValueError(f'cluster {c} outside [0, {self.k})')
        return c


def cluster(index, k, init=None, seed=0, max_iter=50, n_init=1):
    """CubeIndex.cluster (cubesim.py documents it)."""
    k, init, max_iter, n_init = check_cluster_args(index.N, k, init, max_iter, n_init)
    dev = index.dev
    best = None
    with index.lock:
        N = index.N
        if k > N:
            raise ValueError(f'k = {k} is above the {N} cubes of the index')
        for r in range(n_init if init is None else 1):
            ids = init if init is not None else initial_ids(N, k, seed, r)
            ws = index._ws.get(L.lib().cc_cube_cluster_ws_size(N, LATENT, k, 0), dev)
            ids_d = upload(ids, dev)
            lab = torch.empty(N, device=dev, dtype=torch.int32)
            dist = torch.empty(N, device=dev, dtype=torch.float32)
            cent = torch.empty(k, LATENT, device=dev, dtype=torch.float32)
            tail = torch.empty(k + max_iter + 2, device=dev, dtype=torch.int32)   # sizes, changed, n_iter
            L.call('cc_cube_cluster', L.ptr(index._buf), index.capacity, N, LATENT, k, L.ptr(ids_d), max_iter,
                   L.ptr(ws), L.ptr(lab), L.ptr(dist), L.ptr(cent), L.ptr(tail), L.ptr(tail[k:]), L.ptr(tail[-1:]),
                   L.stream_ptr())
            host = [index._stage.fresh(t) for t in (lab, dist, cent, tail)]
            torch.cuda.current_stream().synchronize()
            lab_h, dist_h, cent_h, tail_h = (h.numpy().copy() for h in host)
            del host
            got = CubeClusters(index, ids.copy(), lab_h, dist_h, cent, cent_h, tail_h[:k], tail_h[k:-1], tail_h[-1])
            if best is None or got.objective > best.objective:       # equal objectives: the lower restart
                best = got
    return best
