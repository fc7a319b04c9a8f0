"""Similar cubes: the encoder's 64-float latent of whole cubes, kept on the device as a
normalised index (cc_cube_index_put), and the exact k nearest cubes of member or fresh cubes over it
(cc_cube_neighbours: card similarity's pinned cosine distance, ascending, equal distances lower cube
id first).  The index is normalised once, when a cube is put, and a search's workspace does not
grow with queries x corpus."""
import threading

import numpy as np
import torch

from . import _lib as L
from .launches import Staging, Workspace, mark, pipelined, row_spans, upload, ws_elems
from .recommender import check_card_ids

LATENT = 64   # the encoder's output width (cc_infer_encode_fp32)


def _card_lists(cubes):
    return [np.asarray(c, np.int64).reshape(-1) for c in cubes]


class _Latents:
    """What CubeIndex needs of a Recommender when its rows are given as latents: no encoder."""
    V, d, params = 0, 0, None

    def __init__(self, device):
        self.dev = torch.device(device)


class CubeIndex:
    """Cubes (card-id lists) encoded by a model's encoder and resident on its device.  Cube ids are
    positions: the constructor's cubes are 0..len(cubes)-1, `add` appends.  capacity (default
    len(cubes), at least 1) is fixed: the index is allocated once.  Like similarity.py, every call
    runs on the caller's current stream, holds the index's lock and has waited for that stream
    when it returns."""

    def __init__(self, model_or_recommender, cubes=(), capacity=None, rows_per_launch=4096):
        rec = model_or_recommender.recommender() if hasattr(model_or_recommender, 'recommender') \
            else model_or_recommender
        self.rec, self.V, self.dev = rec, rec.V, rec.dev
        inputs = _card_lists(cubes)
        check_card_ids(inputs, self.V)
        self.capacity = max(1, len(inputs)) if capacity is None else int(capacity)
        if self.capacity < 1:
            raise ValueError(f'capacity {self.capacity} below 1')
        self.N = 0
        self.lock = threading.Lock()      # construction, add and the searches: one at a time
        self._buf = None                  # the index, allocated by the first put
        self._ws, self._stage = Workspace(), Staging()
        self._append(inputs, rows_per_launch)

    def __len__(self):
        return self.N

    # ------------------------------------------------------------------ building
    def _encode(self, inputs):
        """model.encoder on card-id arrays (checked) -> [R, 64] fp32 on the device, queued on the
        current stream without waiting: encode_lists' packing and entry."""
        rec, dev, R = self.rec, self.dev, len(inputs)
        lists = [np.unique(ci).astype(np.int32) for ci in inputs]
        row_ptr = np.zeros(R + 1, np.int32)
        row_ptr[1:] = np.cumsum([len(l) for l in lists])
        max_n = max([len(l) for l in lists], default=0)
        idx = np.concatenate(lists) if R else np.zeros(0, np.int32)
        rp, ix = upload(row_ptr, dev), upload(idx.astype(np.int32), dev)
        z = torch.zeros(R, LATENT, device=dev, dtype=torch.float32)
        ws = torch.empty(ws_elems(L.lib().cc_infer_encode_ws_size(R, rec.d, max_n)), device=dev, dtype=torch.int32)
        L.call('cc_infer_encode_fp32', L.ptr(rec.params), rec.V, rec.d, R, L.ptr(rp), L.ptr(ix), max_n,
               L.ptr(ws), L.ptr(z), L.stream_ptr())
        return z

    def _append(self, inputs, rows_per_launch, latents=None):
        """Encode the (checked) cubes, or take `latents` [R, 64] (device, fp32) as they are, and put
        them behind the last cube; the new ids."""
        R = len(inputs) if latents is None else int(latents.shape[0])
        if self.N + R > self.capacity:
            raise ValueError(f'{R} more cubes do not fit: {self.N} of capacity {self.capacity} are in use')
        if R == 0:
            return range(self.N, self.N)
        with self.lock:
            if self._buf is None:
                size = L.lib().cc_cube_index_size(self.capacity, LATENT)
                self._buf = torch.empty(ws_elems(size), device=self.dev, dtype=torch.int32)
            n0 = self.N
            for r0, r1 in row_spans(R, rows_per_launch):
                z = self._encode(inputs[r0:r1]) if latents is None else latents[r0:r1]
                L.call('cc_cube_index_put', L.ptr(self._buf), self.capacity, LATENT, n0 + r0, r1 - r0, L.ptr(z),
                       L.stream_ptr())
            torch.cuda.current_stream().synchronize()     # the index is ready for any stream
            self.N = n0 + R
        return range(n0, n0 + R)

    @classmethod
    def from_latents(cls, z, capacity=None, device='cuda'):
        """An index of cube latents z [N, 64] (fp32; a tensor or an array) computed elsewhere, e.g.
        by encode_lists.  It has no encoder: neighbours and table work, add and neighbours_of take
        no cubes."""
        z = torch.as_tensor(z, dtype=torch.float32)
        if z.dim() != 2 or z.shape[1] != LATENT:
            raise ValueError(f'latents must be [N, {LATENT}], not {list(z.shape)}')
        dev = z.device if z.is_cuda else torch.device(device)
        z = z.to(dev).contiguous()
        index = cls(_Latents(dev), capacity=max(1, len(z)) if capacity is None else capacity)
        index._append(None, max(1, len(z)), latents=z)
        return index

    def add(self, cubes, rows_per_launch=4096):
        """Append cubes; returns their ids as a range.  More than the capacity holds raises
        ValueError before anything is launched."""
        inputs = _card_lists(cubes)
        check_card_ids(inputs, self.V)
        return self._append(inputs, rows_per_launch)

    # ------------------------------------------------------------------ searching
    def _n_of(self, k, limit):
        """Neighbours per row for a request of k among `limit` candidates; raises above the cap."""
        k = int(k)
        if k <= 0:
            return 0
        cap = int(L.lib().cc_cube_neighbours_max_k())
        if k > cap:
            raise ValueError(f'k = {k} is above cc_cube_neighbours_max_k() = {cap}')
        return max(0, min(k, limit))

    def _search(self, Q, n, qid, fresh, skip, rows_per_launch, chunk):
        """cc_cube_neighbours in launches of up to rows_per_launch rows.  qid / skip: int32 [Q] or
        None; fresh: card-id arrays of fresh cubes (encoded per launch) or None."""
        out_i, out_d = np.empty((Q, n), np.int32), np.empty((Q, n), np.float32)
        chunk = int(chunk)
        if chunk < 0 or chunk % 64:
            raise ValueError(f'chunk {chunk} is not 0 or a positive multiple of 64')
        if Q == 0 or n == 0:
            return out_i, out_d
        dev = self.dev

        def launch(r0, r1, turn):
            Rc = r1 - r0
            ws = self._ws.get(L.lib().cc_cube_neighbours_ws_size(N, LATENT, Rc, n, chunk), dev)
            q_d = upload(qid[r0:r1], dev) if qid is not None else None
            s_d = upload(skip[r0:r1], dev) if skip is not None else None
            z_d = self._encode(fresh[r0:r1]) if fresh is not None else None
            idx = torch.empty(Rc, n, device=dev, dtype=torch.int32)
            dist = torch.empty(Rc, n, device=dev, dtype=torch.float32)
            L.call('cc_cube_neighbours', L.ptr(self._buf), self.capacity, N, LATENT, Rc, L.ptr(q_d), L.ptr(z_d),
                   L.ptr(s_d), n, chunk, L.ptr(ws), L.ptr(idx), L.ptr(dist), L.stream_ptr())
            return (self._stage.fresh(idx), self._stage.fresh(dist)), mark()

        def collect(r0, r1, host):
            out_i[r0:r1] = host[0].numpy()
            out_d[r0:r1] = host[1].numpy()

        with self.lock:
            N = self.N
            last = pipelined(row_spans(Q, rows_per_launch), launch, collect)
            torch.cuda.current_stream().synchronize()   # the workspace is free for the next caller's stream
            del last                  # only now (launches.pipelined)
        return out_i, out_d

    def neighbours(self, ids, k, exclude_self=True, rows_per_launch=512, chunk=0):
        """The k nearest cubes of every member cube of ids (duplicates allowed):
        (indices int32 [Q, n], dists float32 [Q, n]), n = min(k, N - 1) without the cube itself
        (exclude_self), else min(k, N).  Every row is the same bits whatever rows_per_launch, chunk
        (corpus cubes per device pass: 0 for the default, else a multiple of 64), order or batch it
        falls into.  An id outside [0, N) raises ValueError before anything is launched, as does a
        k above cc_cube_neighbours_max_k(); k <= 0 or no ids give [Q, 0] arrays."""
        q = np.asarray(list(ids) if isinstance(ids, range) else ids, np.int64).reshape(-1)
        N = self.N
        bad = np.flatnonzero((q < 0) | (q >= N))
        if len(bad):
            raise ValueError(f'query {int(bad[0])}: cube id {int(q[bad[0]])} outside [0, {N})')
        n = self._n_of(k, N - 1 if exclude_self else N)
        q32 = q.astype(np.int32)
        return self._search(len(q), n, q32, None, q32 if exclude_self else None, rows_per_launch, chunk)

    def neighbours_of(self, cubes, k, rows_per_launch=512, chunk=0):
        """`neighbours` for fresh cubes given as card-id lists, encoded on the device: nothing is
        left out, n = min(k, N).  A member cube asked this way gets the bits
        neighbours([j], exclude_self=False) returns."""
        inputs = _card_lists(cubes)
        check_card_ids(inputs, self.V)
        n = self._n_of(k, self.N)
        return self._search(len(inputs), n, None, inputs, None, rows_per_launch, chunk)

    def table(self, k, rows_per_launch=512, chunk=0):
        """neighbours(range(N), k): every cube's nearest cubes."""
        return self.neighbours(np.arange(self.N, dtype=np.int64), k, rows_per_launch=rows_per_launch, chunk=chunk)

    # ------------------------------------------------------------------ grouping
    def cluster(self, k, init=None, seed=0, max_iter=50, n_init=1):
        """The cubes [0, N) in k archetypes: deterministic spherical k-means, all
        iterations on the device -> cubecluster.CubeClusters.  init: k member ids to start from
        (duplicates allowed); without it restart r draws
        np.random.default_rng(seed + r).choice(N, k, replace=False), and of n_init restarts the one
        with the highest objective is kept, the lower r of equal ones.  The result's every bit is
        fixed by the index, k, the initial ids and max_iter.  k outside 1..min(N,
        cc_cube_cluster_max_k()), a negative max_iter, n_init below 1 or a bad init raise ValueError
        before anything is launched."""
        from . import cubecluster
        return cubecluster.cluster(self, k, init=init, seed=seed, max_iter=max_iter, n_init=n_init)
