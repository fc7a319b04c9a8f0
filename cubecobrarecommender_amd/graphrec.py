"""The co-occurrence baseline on the GPU: additions, cuts and held-out ranks from the card graph.

Replaces ``simple_recs`` (src/scripts/recommend.py:7-18) and ``simple_cuts``
(src/scripts/cut_cards.py:7-18): score every card by the sum of the co-occurrence rows of the
cube's cards, recommend the highest-scoring missing cards and cut the lowest-scoring cube cards.
The graph M (the f64 ``output/full_adj_mtx.npy``, or the matrix ``cc_adjacency`` left on the device)
stays resident in HBM; cc_graph_rec_f64 (csrc/graphrec.hip) gathers and sums the rows in a pinned
order and ranks on the device.  The pinned order is ``M[S].sum(axis=0)`` of a C-contiguous M with
the cube's own diagonal entries taken as 0; the reference's ``adj[contains][:, missing].sum(0)``
sums the same numbers pairwise and differs in the last bits.
"""
import threading

import numpy as np
import torch

from . import _lib as L
from .launches import Staging, Workspace, mark, pipelined, row_spans, target_ranks_rows, upload
from .recommender import RANK_STAGING_BYTES, check_card_ids, pack_cubes, pack_targets


def graph_rank_rows_per_launch(V, A, rows_per_launch, want_vals=True, want_scores=False,
                               budget_bytes=RANK_STAGING_BYTES):
    """Rows per launch of rank_many (pure host code): at most rows_per_launch, at least 1, and as
    many as keep one launch's pinned staging within budget_bytes.  A row stages n_add and A
    additions (int32), A values (f64) unless dropped, and V scores (f64) on request; the cut
    values (one f64 per cube card) are small beside them and not counted."""
    per_row = 4 + 4 * int(A) + (8 * int(A) if want_vals else 0) + (8 * int(V) if want_scores else 0)
    return max(1, min(int(rows_per_launch), int(budget_bytes) // per_row))


def result_rows(Rc, A, row_ptr, idx, ints, addv, cutv, scores):
    """The result dicts of one launch of Rc rows from its host arrays, the caller's own copies
    (addv [Rc, A] and scores [Rc, V] may be None); the cube's cards are put into cut order here."""
    nadd, adds = ints[:Rc].tolist(), ints[Rc:].reshape(Rc, A)
    rows = []
    for r in range(Rc):
        k = nadd[r]
        ids, vals = idx[row_ptr[r]:row_ptr[r + 1]], cutv[row_ptr[r]:row_ptr[r + 1]]
        order = np.argsort(vals, kind='stable')     # about 360 values: the host's job
        o = {'additions': adds[r, :k]}
        if addv is not None:
            o['add_vals'] = addv[r, :k]
        o['cuts'], o['cut_vals'] = ids[order], vals[order]
        if scores is not None:
            o['scores'] = scores[r]
        rows.append(o)
    return rows


class GraphRecommender:
    def __init__(self, adj, device='cuda'):
        """adj: the graph, an f64 numpy [V, V] (uploaded once) or an f64 device tensor [V, V] whose
        rows are contiguous (used in place: a row pitch above V is fine)."""
        L.lib()
        if torch.is_tensor(adj):
            self.dev = adj.device
            self.adj = adj
        else:
            self.dev = torch.device(device)
            a = np.asarray(adj)
            if a.dtype != np.float64:
                raise ValueError('the adjacency matrix must be float64')
            self.adj = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        a = self.adj
        if a.dtype != torch.float64 or a.dim() != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
            raise ValueError('the adjacency matrix must be a square float64 matrix')
        if a.shape[1] > 1 and a.stride(1) != 1 or a.shape[0] > 1 and a.stride(0) < a.shape[1]:
            raise ValueError('the rows of the adjacency matrix must be contiguous')
        self.V = int(a.shape[0])
        self.ld = int(a.stride(0)) if self.V > 1 else self.V
        self.stream = torch.cuda.Stream(device=self.dev)
        self.lock = threading.Lock()
        # one workspace serves every entry: cc_graph_rank_ws_size is never below cc_graph_rec_ws_size
        # for the same rows (tests/test_graph_rank_host.py), and the lock admits one call at a time
        self._ws = Workspace()
        self._rank_pins = Staging()     # pinned staging; rank_many keeps two sets in it
        # requests run on the recommender's own stream: the matrix (an upload, or cc_adjacency on
        # another stream) must be complete before they can
        torch.cuda.synchronize(self.dev)

    @classmethod
    def from_cubes(cls, indptr, indices, V, device='cuda'):
        """The graph of CSR cube lists, built on the device (adjacency.py: cc_adjacency's M)."""
        from .adjacency import adjacency_gpu
        return cls(adjacency_gpu(indptr, indices, V, ('M',), device=device)['M'])

    # ------------------------------------------------------------------ additions and cuts
    def recommend(self, cube_indices, amount, want_scores=False):
        """`recommend_many` for one cube."""
        return self.recommend_many([cube_indices], amount, want_scores=want_scores)[0]

    def recommend_many(self, cubes, amount, want_scores=False, rows_per_launch=512):
        """simple_recs and simple_cuts for every cube of `cubes` (card-index lists; duplicates
        collapse, as in the reference's 0/1 cube vector), in launches of up to rows_per_launch
        rows.  Returns a list of dicts:

          additions int32, add_vals f64   the min(max(amount, 1), V - n) highest-scoring cards
                                          outside the cube, descending, equal scores higher index
                                          first (argsort(kind='stable')[::-1]), and their scores
          cuts int32, cut_vals f64        the cube's distinct cards in cut order: ascending score,
                                          equal scores lower index first, and their scores
          scores f64 [V]                  on request: every card's score

        A row's bits do not depend on the batch or the launch it falls into.  An id outside
        [0, V) or an amount above cc_graph_rec_max_amount() raises ValueError before anything is
        launched (rank_many takes any amount and ranks every card; target_ranks serves
        evaluation)."""
        amount = int(amount)
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        R = len(inputs)
        V = self.V
        check_card_ids(inputs, V)
        cap = int(L.lib().cc_graph_rec_max_amount())
        if amount > cap:
            raise ValueError(f'amount {amount} above the graph path\'s limit of {cap}')
        if R == 0:
            return []
        A = max(amount, 1)
        dev, stage = self.dev, self._rank_pins
        out = []

        def launch(r0, r1, turn):
            """Pack rows r0..r1, queue their launch and the copies of its results to fresh pinned
            memory; no waiting."""
            row_ptr, idx, max_n, _, _ = pack_cubes(inputs[r0:r1], V)
            Rc, nnz = r1 - r0, len(idx)
            ws = self._ws.get(L.lib().cc_graph_rec_ws_size(V, Rc, max_n), dev)
            rp_d, ix_d = upload(row_ptr, dev), upload(idx, dev)
            ints = torch.empty(Rc * (1 + A), device=dev, dtype=torch.int32)            # n_add, additions
            flts = torch.empty(Rc * A + max(nnz, 1), device=dev, dtype=torch.float64)  # add_vals, cut_vals
            scores = torch.empty(Rc, V, device=dev, dtype=torch.float64) if want_scores else None
            L.call('cc_graph_rec_f64', L.ptr(self.adj), self.ld, V, Rc, L.ptr(rp_d), L.ptr(ix_d), max_n,
                   amount, L.ptr(ws), L.ptr(ints), L.ptr(ints[Rc:]), L.ptr(flts), L.ptr(flts[Rc * A:]),
                   L.ptr(scores), L.stream_ptr(self.stream))
            host = [stage.fresh(t) for t in ((ints, flts, scores) if want_scores else (ints, flts))]
            return (row_ptr, idx, host), mark(self.stream)

        def collect(r0, r1, payload):
            row_ptr, idx, host = payload
            Rc = r1 - r0
            ints, flts = host[0].numpy().copy(), host[1].numpy().copy()
            out.extend(result_rows(Rc, A, row_ptr, idx, ints, flts[:Rc * A].reshape(Rc, A), flts[Rc * A:],
                                   host[2].numpy().copy() if want_scores else None))

        with self.lock, torch.cuda.stream(self.stream):
            pipelined(row_spans(R, rows_per_launch), launch, collect)
        return out

    # ------------------------------------------------------------------ every card, ranked
    def rank_many(self, cubes, amount=None, want_vals=True, want_scores=False, rows_per_launch=512):
        """`recommend_many` for any amount; amount=None ranks every card (simple_recs' complete
        list).  cc_graph_rank_f64: the scoring pass, then one sorting workgroup per row.  Returns
        the list of dicts of recommend_many, bit for bit where both are defined: additions int32 of
        length min(max(amount, 1), V - n), add_vals f64 (absent with want_vals=False: two thirds
        of the result bytes), cuts / cut_vals in cut order, scores on request.  Launches are capped
        by graph_rank_rows_per_launch, and their results pass through two pinned staging sets that
        the GraphRecommender keeps.  An id outside [0, V) raises ValueError naming the cube before
        anything is launched."""
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        R = len(inputs)
        V = self.V
        check_card_ids(inputs, V)
        if R == 0:
            return []
        amount = V if amount is None else int(amount)
        A = min(max(amount, 1), V)
        rows_per_launch = graph_rank_rows_per_launch(V, A, rows_per_launch, want_vals, want_scores)
        dev, stage = self.dev, self._rank_pins
        out = []

        def launch(r0, r1, turn):
            """Pack rows r0..r1, queue their launch and the copies of its results to the kept
            staging set of the turn's parity; no waiting."""
            row_ptr, idx, max_n, _, _ = pack_cubes(inputs[r0:r1], V)
            Rc, nnz = r1 - r0, len(idx)
            ws = self._ws.get(L.lib().cc_graph_rank_ws_size(V, Rc, max_n), dev)
            rp_d, ix_d = upload(row_ptr, dev), upload(idx, dev)
            ints = torch.empty(Rc * (1 + A), device=dev, dtype=torch.int32)            # n_add, additions
            vals = torch.empty(Rc * A, device=dev, dtype=torch.float64) if want_vals else None
            cutv = torch.empty(max(nnz, 1), device=dev, dtype=torch.float64)
            scores = torch.empty(Rc, V, device=dev, dtype=torch.float64) if want_scores else None
            L.call('cc_graph_rank_f64', L.ptr(self.adj), self.ld, V, Rc, L.ptr(rp_d), L.ptr(ix_d), max_n,
                   amount, L.ptr(ws), L.ptr(ints), L.ptr(ints[Rc:]), L.ptr(vals), L.ptr(cutv),
                   L.ptr(scores), L.stream_ptr(self.stream))
            host = {name: stage.kept(t, (turn & 1, name))
                    for name, t in (('ints', ints), ('vals', vals), ('cutv', cutv), ('scores', scores))
                    if t is not None}
            return (row_ptr, idx, host), mark(self.stream)

        def collect(r0, r1, payload):
            row_ptr, idx, host = payload
            Rc = r1 - r0
            got = {name: t.numpy().copy() for name, t in host.items()}     # out of the pinned staging
            out.extend(result_rows(Rc, A, row_ptr, idx, got['ints'],
                                   got['vals'].reshape(Rc, A) if want_vals else None, got['cutv'],
                                   got.get('scores')))

        with self.lock, torch.cuda.stream(self.stream):
            pipelined(row_spans(R, rows_per_launch), launch, collect)
        return out

    # ------------------------------------------------------------------ held-out evaluation
    def target_ranks(self, cubes, targets, cutoffs=(), rows_per_launch=512):
        """Where the cards of targets[r] land in the full ranking of cube r's additions, without
        ranking anything (cc_graph_rec_target_ranks_f64: the scoring pass, then a count per
        target).  Arguments and return shape of Recommender.target_ranks, so
        evaluate.evaluate_holdout takes a GraphRecommender as its model: (ranks, vals, hits) with
        int32 ranks and float64 scores per cube in the caller's target order, hits None without
        cutoffs, else the device's uint64 counters [len(cutoffs) + 2]."""
        cutoffs = [int(k) for k in cutoffs]
        if len(cutoffs) > 8:
            raise ValueError('at most 8 cutoffs')
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        R = len(inputs)
        V = self.V
        check_card_ids(inputs, V)
        tgt_ptr, tgt = pack_targets(targets, inputs, V)
        if R == 0:
            return [], [], (np.zeros(len(cutoffs) + 2, np.uint64) if cutoffs else None)
        dev = self.dev

        def call(s):
            ws = self._ws.get(L.lib().cc_graph_rec_ws_size(V, s.Rc, s.max_n), dev)
            L.call('cc_graph_rec_target_ranks_f64', L.ptr(self.adj), self.ld, V, s.Rc, L.ptr(s.rp), L.ptr(s.ix),
                   s.max_n, L.ptr(s.tp), L.ptr(s.tg), L.ptr(s.cut), s.nk, L.ptr(ws), L.ptr(s.rk), L.ptr(s.tv),
                   L.ptr(s.hits), L.ptr(s.cuts), None, L.stream_ptr(self.stream))

        with self.lock, torch.cuda.stream(self.stream):
            return target_ranks_rows(pack_cubes, inputs, V, tgt_ptr, tgt, cutoffs, rows_per_launch, dev,
                                     self.stream, self._rank_pins, torch.float64, call)
