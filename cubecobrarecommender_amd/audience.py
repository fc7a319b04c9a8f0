"""Card audience: which cubes most want this card?  A corpus of cubes kept on the
device as the decoder's last hidden rows with the cubes' card lists beside them (cc_audience_put),
and per query card the k corpus cubes with the highest p(card | cube) among those that do not
play it yet (cc_audience_fp32).  Every probability is the bits recommend_many reports for that cube
and card; the output layer is computed at the asked cards only, and a query's workspace does not
grow with cards x corpus."""
import threading

import numpy as np
import torch

from . import _lib as L
from .launches import Staging, Workspace, mark, pipelined, row_spans, upload, ws_elems
from .recommender import pack_cubes

PUT_ROWS = 65535      # rows of one cc_audience_put
QUERY_CARDS = 4096    # cards of one cc_audience_fp32
MAX_CHUNK = 1 << 20


class CubeCorpus:
    """Cubes (card-id lists) under a model's forward pass, resident on its device.  Cube ids are
    positions: the constructor's cubes are 0..len(cubes)-1, `add` appends.  capacity (default
    len(cubes), at least 1) and card_capacity (default the given cubes' total distinct cards, at
    least 1) are fixed: the corpus is allocated once.  Like CubeIndex, every call runs on the
    caller's current stream, holds the corpus's lock and has waited for that stream when it
    returns."""

    def __init__(self, model_or_recommender, cubes=(), capacity=None, card_capacity=None, rows_per_launch=4096):
        rec = model_or_recommender.recommender() if hasattr(model_or_recommender, 'recommender') \
            else model_or_recommender
        self.rec, self.V, self.d, self.dev = rec, rec.V, rec.d, rec.dev
        row_ptr, idx, _, _, _ = pack_cubes(cubes, self.V)
        self.capacity = max(1, len(row_ptr) - 1) if capacity is None else int(capacity)
        self.card_capacity = max(1, len(idx)) if card_capacity is None else int(card_capacity)
        if self.capacity < 1:
            raise ValueError(f'capacity {self.capacity} below 1')
        if self.card_capacity < 1:
            raise ValueError(f'card_capacity {self.card_capacity} below 1')
        self.N, self.nnz = 0, 0
        self.lock = threading.Lock()      # construction, add and the queries: one at a time
        self._buf = None                  # the corpus, allocated by the first put
        self._ws, self._stage = Workspace(), Staging()
        self._append(row_ptr, idx, rows_per_launch)

    def __len__(self):
        return self.N

    # ------------------------------------------------------------------ building
    def _append(self, row_ptr, idx, rows_per_launch):
        """Put the cubes of a checked CSR (pack_cubes) behind the last cube; the new ids."""
        R, nnz = len(row_ptr) - 1, len(idx)
        if self.N + R > self.capacity:
            raise ValueError(f'{R} more cubes do not fit: {self.N} of capacity {self.capacity} are in use')
        if self.nnz + nnz > self.card_capacity:
            raise ValueError(f'{nnz} more cards do not fit: {self.nnz} of card_capacity {self.card_capacity} '
                             f'are in use')
        if R == 0:
            return range(self.N, self.N)
        rec, dev, lib = self.rec, self.dev, L.lib()
        with self.lock:
            if self._buf is None:
                size = lib.cc_audience_corpus_size(self.capacity, self.card_capacity, self.d)
                self._buf = torch.empty(ws_elems(size), device=dev, dtype=torch.int32)
            n0, nnz0 = self.N, self.nnz
            for r0, r1 in row_spans(R, min(max(1, int(rows_per_launch)), PUT_ROWS)):
                lo, hi = int(row_ptr[r0]), int(row_ptr[r1])
                rp = (row_ptr[r0:r1 + 1] - row_ptr[r0]).astype(np.int32)
                max_n = int(np.diff(rp).max())
                ws = self._ws.get(lib.cc_audience_put_ws_size(r1 - r0, self.d, max_n), dev)
                rp_d, ix_d = upload(rp, dev), upload(idx[lo:hi], dev)     # both alive until the put is queued
                L.call('cc_audience_put', L.ptr(rec.params), self.V, self.d, L.ptr(self._buf), self.capacity,
                       self.card_capacity, n0 + r0, nnz0 + lo, r1 - r0, L.ptr(rp_d), L.ptr(ix_d), hi - lo, max_n,
                       L.ptr(ws), L.stream_ptr())
            torch.cuda.current_stream().synchronize()     # the corpus is ready for any stream
            self.N, self.nnz = n0 + R, nnz0 + nnz
        return range(n0, n0 + R)

    def add(self, cubes, rows_per_launch=4096):
        """Append cubes; returns their ids as a range.  More cubes than capacity or more distinct
        cards than card_capacity hold, or a card outside [0, V), raise ValueError before anything
        is launched."""
        row_ptr, idx, _, _, _ = pack_cubes(cubes, self.V)
        return self._append(row_ptr, idx, rows_per_launch)

    # ------------------------------------------------------------------ asking
    def audience(self, cards, k, include_members=False, threshold=0.5, rows_per_launch=64, chunk=0):
        """Per query card (duplicates allowed, independent rows) the corpus cubes that want it
        most: a dict of
          cubes int32 [T, n], probs float32 [T, n]   n = min(k, N): the first found[t] entries are
              cube ids and p(card | cube), descending p, equal p lower cube id first; then -1 / 0
          found, members, candidates, above int32 [T]   found = min(k, candidates); members: cubes
              that hold the card; candidates: the cubes ranked, those that do not hold it (every
              cube with include_members); above: candidates with p >= threshold (fp32).
        Every row is the same bits whatever rows_per_launch (cards per launch), chunk (corpus cubes
        per device pass: 0 for the default, else a multiple of 64) or batch it falls into.  A card
        outside [0, V), a k above cc_audience_max_k(), a threshold outside [0, 1] and a bad chunk
        raise ValueError before anything is launched.  k <= 0 gives [T, 0] arrays beside the
        counts; an empty corpus or no cards launch nothing."""
        q = np.asarray(list(cards) if isinstance(cards, range) else cards, np.int64).reshape(-1)
        bad = np.flatnonzero((q < 0) | (q >= self.V))
        if len(bad):
            raise ValueError(f'query {int(bad[0])}: card {int(q[bad[0]])} outside [0, {self.V})')
        k, chunk = int(k), int(chunk)
        cap = int(L.lib().cc_audience_max_k())
        if k > cap:
            raise ValueError(f'k = {k} is above cc_audience_max_k() = {cap}')
        threshold = float(threshold)
        if not 0.0 <= threshold <= 1.0:            # (NaN fails both comparisons)
            raise ValueError(f'threshold {threshold} outside [0, 1]')
        if chunk < 0 or chunk % 64 or chunk > MAX_CHUNK:
            raise ValueError(f'chunk {chunk} is not 0 or a positive multiple of 64 up to {MAX_CHUNK}')
        T, dev, rec = len(q), self.dev, self.rec
        q32 = q.astype(np.int32)
        thr = float(np.float32(threshold))

        with self.lock:
            N = self.N
            n = max(0, min(k, N))
            kk = max(n, 1)                         # k <= 0: one column is computed for the counts
            out_i, out_p = np.empty((T, n), np.int32), np.empty((T, n), np.float32)
            counts = np.zeros((T, 3), np.int32)
            if T == 0 or N == 0:
                return self._result(out_i, out_p, counts, n)

            def launch(r0, r1, turn):
                Tc = r1 - r0
                ws = self._ws.get(L.lib().cc_audience_ws_size(N, self.d, Tc, kk, chunk), dev)
                idx = torch.empty(Tc, kk, device=dev, dtype=torch.int32)
                p = torch.empty(Tc, kk, device=dev, dtype=torch.float32)
                cnt = torch.empty(Tc, 3, device=dev, dtype=torch.int32)
                c_d = upload(q32[r0:r1], dev)
                L.call('cc_audience_fp32', L.ptr(rec.params), self.V, self.d, L.ptr(self._buf), self.capacity, N, Tc,
                       L.ptr(c_d), kk, chunk, 1 if include_members else 0, thr, L.ptr(ws), L.ptr(idx), L.ptr(p),
                       L.ptr(cnt), L.stream_ptr())
                return (self._stage.fresh(idx), self._stage.fresh(p), self._stage.fresh(cnt)), mark()

            def collect(r0, r1, host):
                out_i[r0:r1] = host[0].numpy()[:, :n]
                out_p[r0:r1] = host[1].numpy()[:, :n]
                counts[r0:r1] = host[2].numpy()

            last = pipelined(row_spans(T, min(max(1, int(rows_per_launch)), QUERY_CARDS)), launch, collect)
            torch.cuda.current_stream().synchronize()   # the workspace is free for the next caller's stream
            del last                  # only now (launches.pipelined)
        return self._result(out_i, out_p, counts, n)

    def group_cards(self, labels, m, kind='lift', min_count=1, G=None, counts=False, rows_per_launch=1 << 20):
        """The corpus's cubes grouped by labels (one per cube, -1: ignored) -> groupcards.GroupCards
        (DESIGN §4.13), the integers groupcards.group_cards gives for the same cubes, counted from
        the resident card lists: no card is uploaded.  len(labels) must equal len(corpus);
        rows_per_launch: corpus cubes per launch (the result does not depend on it)."""
        from . import groupcards
        return groupcards.corpus_group_cards(self, labels, m, kind=kind, min_count=min_count, G=G, counts=counts,
                                             rows_per_launch=rows_per_launch)

    @staticmethod
    def _result(out_i, out_p, counts, n):
        members, candidates, above = (np.ascontiguousarray(counts[:, j]) for j in range(3))
        return {'cubes': out_i, 'probs': out_p, 'found': np.minimum(candidates, n).astype(np.int32),
                'members': members, 'candidates': candidates, 'above': above}
