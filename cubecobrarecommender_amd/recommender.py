"""Resident-model recommend path: fp32 forward (bit-exact pinned order) + top-N on the GPU.

Replaces the hot part of ``src/scripts/ml_recommend.py:78-108`` and
``web/ml_recommend_web.py:39-64``: ``model.encoder(x)`` -> ``model.decoder(z)`` -> ``argsort``
-> additions / cuts.  Unlike the reference web path (which reloads the ~390 MB SavedModel on every
request, ml_recommend_web.py:37) the weights stay resident in HBM; requests are serialised per
``Recommender`` with a lock (Flask runs threaded, web/__init__.py:41) and run on its own stream.
"""
import threading

import numpy as np
import torch

from . import _lib as L
from .launches import Staging, Workspace, mark, pipelined, row_spans, target_ranks_rows, upload, ws_elems
from .layout import Layout

GRAPH_MAX_IDS = 4096   # cube ids per request the captured graph's H2D carries
RANK_STAGING_BYTES = 128 << 20   # pinned result staging per launch of the full-ranking batched path


def check_card_ids(inputs, V):
    """ValueError unless every id of every array of `inputs` is in [0, V); names the first cube."""
    flat = np.concatenate(inputs) if len(inputs) else np.zeros(0, np.int64)
    if not len(flat) or (flat.min() >= 0 and flat.max() < V):
        return
    for r, ci in enumerate(inputs):
        if len(ci) and (ci.min() < 0 or ci.max() >= V):
            raise ValueError(f'cube {r}: card index outside [0, {V})')


def pack_cubes(cubes, V):
    """R card-index lists -> the CSR that cc_recommend_batch_fp32 takes (pure host code, one sort
    over all rows).

    Returns (row_ptr int32 [R+1], idx int32 [row_ptr[R]], max_n, inputs, slot): row r of the CSR is
    the sorted distinct ids of cubes[r]; inputs[r] is cubes[r] as an int64 array in the caller's
    order, duplicates kept; slot [sum of len(inputs[r])] is, for every input entry in turn, the
    position of its card in idx.  Raises ValueError for an id outside [0, V): the kernels index
    the weights with these ids unchecked."""
    inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
    R = len(inputs)
    lens = np.fromiter((len(ci) for ci in inputs), np.int64, R)
    flat = np.concatenate(inputs) if R else np.zeros(0, np.int64)
    rows = np.repeat(np.arange(R, dtype=np.int64), lens)
    if len(flat) and (flat.min() < 0 or flat.max() >= V):
        check_card_ids(inputs, V)
    key = rows * V + flat                        # (row, card): equal entries are duplicates
    order = np.argsort(key)
    skey = key[order]
    first = np.ones(len(skey), bool)
    first[1:] = skey[1:] != skey[:-1]
    ukey = skey[first]
    slot = np.empty(len(skey), np.int64)
    slot[order] = np.cumsum(first) - 1
    counts = np.bincount(ukey // V, minlength=R) if R else np.zeros(0, np.int64)
    row_ptr = np.zeros(R + 1, np.int32)
    row_ptr[1:] = np.cumsum(counts)
    idx = (ukey % V).astype(np.int32)
    return row_ptr, idx, int(counts.max()) if R else 0, inputs, slot


def pack_targets(targets, inputs, V):
    """R target-card lists -> the target CSR of cc_recommend_batch_target_ranks_fp32 (pure host
    code).  inputs[r] is the visible cube of row r (as pack_cubes returns it).

    Returns (tgt_ptr int32 [R+1], tgt int32 [tgt_ptr[R]]): row r holds targets[r] in the caller's
    order, duplicates kept.  Raises ValueError for a target outside [0, V), and for a target that
    is also a card of its row's cube (it has no rank among the candidates), naming the cube."""
    tl = [np.asarray(t, np.int64).reshape(-1) for t in targets]
    R = len(tl)
    if R != len(inputs):
        raise ValueError(f'{R} target lists for {len(inputs)} cubes')
    check_card_ids(tl, V)
    lens = np.fromiter((len(t) for t in tl), np.int64, R)
    flat = np.concatenate(tl) if R else np.zeros(0, np.int64)
    rows = np.repeat(np.arange(R, dtype=np.int64), lens)
    cube_lens = np.fromiter((len(ci) for ci in inputs), np.int64, R)
    cube_key = np.repeat(np.arange(R, dtype=np.int64), cube_lens) * V + (
        np.concatenate(inputs).astype(np.int64) if R else np.zeros(0, np.int64))
    inside = np.isin(rows * V + flat, cube_key)
    if inside.any():
        at = int(np.flatnonzero(inside)[0])
        raise ValueError(f'cube {int(rows[at])}: target card {int(flat[at])} is in the cube')
    tgt_ptr = np.zeros(R + 1, np.int32)
    tgt_ptr[1:] = np.cumsum(lens)
    return tgt_ptr, flat.astype(np.int32)


def pool_words(ids, V):
    """Card ids -> the pool's bit row, uint32 [ceil(V / 32)] (pure host code): bit j & 31 of word
    j >> 5 set for every id j.  Order does not matter, duplicates collapse, the empty pool is legal;
    bits at or above V stay zero.  Raises ValueError for an id outside [0, V)."""
    V = int(V)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if len(ids) and (ids.min() < 0 or ids.max() >= V):
        bad = ids[(ids < 0) | (ids >= V)][0]
        raise ValueError(f'pool card {int(bad)} outside [0, {V})')
    words = np.zeros((V + 31) // 32, np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return words


class CardPool:
    """A set of card ids that narrows the candidates of a ranking call: the sorted distinct `ids`,
    their number `size`, the card count `V` the pool was built for, its bit row `words`
    (pool_words) and, from Recommender.card_pool, the same words on the device (`words_dev`).
    Immutable after construction: one pool serves any number of calls and threads."""

    def __init__(self, ids, V, words_dev=None):
        self.V = int(V)
        self.words = pool_words(ids, self.V)
        self.ids = np.unique(np.asarray(ids, np.int64).reshape(-1))
        self.size = len(self.ids)
        self.words_dev = words_dev

    def contains(self, cards):
        """bool array: which of the card ids `cards` are in the pool (none outside [0, V) is)."""
        cards = np.asarray(cards, np.int64)
        ok = (cards >= 0) & (cards < self.V)
        c = np.where(ok, cards, 0)
        return ok & ((self.words[c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


def pools_per_row(pool, R):
    """The `pool` argument of a ranking call (not None) as a list of R entries, each a CardPool or
    None.  Raises ValueError for a sequence of another length or an entry of another type."""
    per_row = [pool] * R if isinstance(pool, CardPool) else list(pool)
    if len(per_row) != R:
        raise ValueError(f'{len(per_row)} pools for {R} cubes')
    for r, p in enumerate(per_row):
        if p is not None and not isinstance(p, CardPool):
            raise ValueError(f'cube {r}: the pool is {type(p).__name__}, not a CardPool or None')
    return per_row


def resolve_pools(pool, R, V):
    """The `pool` argument of a ranking call -> (pools, pool_of_row), or (None, None) for no pool
    at all (pure host code).  `pool` is None, one CardPool for every row, or a sequence of R
    entries, each a CardPool or None.  pools: the call's distinct CardPools in order of first use;
    pool_of_row: int32 [R], row r's index into pools, -1 for a row without one.  Raises ValueError
    for a sequence of another length, an entry that is no CardPool, or a pool built for another V."""
    if pool is None:
        return None, None
    pools, at = [], {}
    pool_of_row = np.full(R, -1, np.int32)
    for r, p in enumerate(pools_per_row(pool, R)):
        if p is None:
            continue
        if p.V != V:
            raise ValueError(f'cube {r}: the pool was built for {p.V} cards, the model has {V}')
        if id(p) not in at:
            at[id(p)] = len(pools)
            pools.append(p)
        pool_of_row[r] = at[id(p)]
    if not pools:
        return None, None
    return pools, pool_of_row


def check_targets_in_pools(targets, pools, pool_of_row):
    """ValueError for the first target card outside its row's pool, naming the cube and the card
    (such a card has no rank among the row's candidates).  Ids are already known to be in [0, V)."""
    for r, t in enumerate(targets):
        if pool_of_row[r] < 0:
            continue
        t = np.asarray(t, np.int64).reshape(-1)
        out = ~pools[pool_of_row[r]].contains(t)
        if out.any():
            raise ValueError(f'cube {r}: target card {int(t[np.flatnonzero(out)[0]])} is outside the pool')


def cuts_in_input_order(cut_csr, slot, inputs):
    """cut_csr (aligned with the CSR's idx) -> per cube, the values in the caller's input order
    with duplicates repeated (pure host code)."""
    vals = np.asarray(cut_csr, np.float32)[slot]
    ends = np.cumsum([len(ci) for ci in inputs])
    return [vals[e - len(ci):e] for ci, e in zip(inputs, ends)]


def rank_rows_per_launch(V, A, rows_per_launch, budget_bytes=RANK_STAGING_BYTES, want_probs=False):
    """Rows per launch of the full-ranking path (pure host code): at most rows_per_launch, at
    least 1, and as many as keep one launch's pinned staging within budget_bytes.  A row stages
    n_add, A additions, A values and up to V cut values (plus V probabilities on request)."""
    per_row = 4 * (1 + 2 * int(A) + int(V) * (2 if want_probs else 1))
    return max(1, min(int(rows_per_launch), int(budget_bytes) // per_row))


class Recommender:
    _graph = None       # the captured request graph, once made (__del__ may meet a half-built object)

    def __init__(self, params_flat, V, d, device='cuda'):
        L.lib()
        self.V, self.d = int(V), int(d)
        self.layout = Layout(V, d)
        self.dev = torch.device(device)
        p = torch.as_tensor(np.asarray(params_flat, np.float32)) if not torch.is_tensor(params_flat) else params_flat
        self.params = p.to(self.dev, torch.float32).contiguous()
        assert self.params.numel() >= self.layout.main_total
        self.stream = torch.cuda.Stream(device=self.dev)
        self.lock = threading.Lock()
        self.probs_dev = torch.zeros(V, device=self.dev, dtype=torch.float32)
        self.ws = torch.zeros(ws_elems(L.lib().cc_recommend_ws_size(V, d)), device=self.dev, dtype=torch.int32)
        # request I/O: req = {n, amount, ids[n]}, res = {n_add, additions, add_vals, cut_vals}
        self.cap = min(V, GRAPH_MAX_IDS)
        self.req_dev = torch.zeros(2 + V, device=self.dev, dtype=torch.int32)
        self.res_dev = torch.zeros(1 + 2 * V + V, device=self.dev, dtype=torch.int32)
        self.pin_req = torch.zeros(2 + V, dtype=torch.int32).pin_memory()
        self.pin_res = torch.zeros(1 + 2 * V + V, dtype=torch.int32).pin_memory()
        self._req_np = self.pin_req.numpy()
        self._res_np = self.pin_res.numpy()
        self._batch_ws = Workspace()    # the batched calls' workspace ...
        self._rank_pins = Staging()     # ... and their pinned staging (kept on the full-ranking path)
        # the request graph runs on the library's own non-blocking stream: every allocation and
        # fill above (issued on torch's stream) must be complete before it can run
        torch.cuda.synchronize(self.dev)

    def __del__(self):
        if self._graph is not None:
            try:
                L.lib().cc_recommend_graph_destroy(self._graph)
            except Exception:
                pass

    def _graph_handle(self):
        if self._graph is None:
            h = L.C.c_void_p()
            L.call('cc_recommend_graph_create', L.ptr(self.params), self.V, self.d, L.ptr(self.pin_req),
                   L.ptr(self.req_dev), self.cap, L.ptr(self.ws), L.ptr(self.probs_dev), L.ptr(self.res_dev),
                   L.C.byref(h))
            self._graph = h
        return self._graph

    # ------------------------------------------------------------------ batched encoder / decoder
    def encode_lists(self, lists):
        """model.encoder(x) for R cubes given as card-index lists -> [R, 64] fp32 (device)."""
        R = len(lists)
        lists = [np.unique(np.asarray(l, np.int64)).astype(np.int32) for l in lists]
        row_ptr = np.zeros(R + 1, np.int32)
        row_ptr[1:] = np.cumsum([len(l) for l in lists])
        max_n = max([len(l) for l in lists], default=0)
        idx = np.concatenate(lists) if R else np.zeros(0, np.int32)
        with torch.cuda.stream(self.stream):
            rp = torch.from_numpy(row_ptr).to(self.dev, non_blocking=True)
            ix = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).to(self.dev, non_blocking=True)
            z = torch.zeros(R, 64, device=self.dev, dtype=torch.float32)
            ws = torch.empty(int(L.lib().cc_infer_encode_ws_size(R, self.d, max_n)) // 4 + 4,
                             device=self.dev, dtype=torch.float32)
            L.call('cc_infer_encode_fp32', L.ptr(self.params), self.V, self.d, R, L.ptr(rp), L.ptr(ix),
                   max_n, L.ptr(ws), L.ptr(z), L.stream_ptr(self.stream))
        self.stream.synchronize()
        return z

    def decode(self, z):
        """model.decoder(z): [R, 64] -> sigmoid probabilities [R, V] fp32 (device)."""
        z = torch.as_tensor(z, dtype=torch.float32).to(self.dev).contiguous()
        R = z.shape[0]
        with torch.cuda.stream(self.stream):
            h3 = torch.zeros(R, self.d, device=self.dev, dtype=torch.float32)
            out = torch.zeros(R, self.V, device=self.dev, dtype=torch.float32)
            L.call('cc_infer_decode_fp32', L.ptr(self.params), self.V, self.d, R, L.ptr(z), L.ptr(h3),
                   L.ptr(out), L.stream_ptr(self.stream))
        self.stream.synchronize()
        return out

    def cube_index(self, cubes, capacity=None):
        """A resident index of `cubes` (card-index lists) for nearest-cube searches
        (cubesim.CubeIndex)."""
        from .cubesim import CubeIndex
        return CubeIndex(self, cubes, capacity=capacity)

    def cube_corpus(self, cubes, capacity=None, card_capacity=None):
        """A resident corpus of `cubes` (card-index lists) under this model's forward pass, for
        "which cubes want this card" (audience.CubeCorpus)."""
        from .audience import CubeCorpus
        return CubeCorpus(self, cubes, capacity=capacity, card_capacity=card_capacity)

    # ------------------------------------------------------------------ card pools
    def card_pool(self, ids):
        """A CardPool of `ids` for this model with its bit row on the device: uploaded once, then
        passed as `pool=` to recommend / recommend_many / target_ranks any number of times.  Raises
        ValueError for an id outside [0, V)."""
        pool = CardPool(ids, self.V)
        pool.words_dev = torch.from_numpy(pool.words.view(np.int32)).to(self.dev)
        return pool

    def _pool_table(self, pools):
        """The call's distinct pools stacked into one device table [n_pools][VW], once per call."""
        def here(t):     # self.dev may carry no index ('cuda'): then any index of its type is taken as it
            return t is not None and t.device.type == self.dev.type and self.dev.index in (None, t.device.index)
        rows = [p.words_dev if here(p.words_dev) else torch.from_numpy(p.words.view(np.int32)).to(self.dev)
                for p in pools]
        return torch.stack(rows).contiguous()

    @staticmethod
    def _pool_args(table, pool_of_row_dev, none=()):
        """The pool arguments of an entry call, (pools, n_pools, pool_of_row), from the call's
        _pool_table and the span's uploaded pool_of_row; `none` without a table (no pools)."""
        return none if table is None else (L.ptr(table), table.shape[0], L.ptr(pool_of_row_dev))

    # ------------------------------------------------------------------ single-cube request
    def recommend(self, cube_indices, amount, want_probs=False, want_order=False, pool=None):
        """ml_recommend.py:78-108 for one cube.  Returns dict with additions (card idx,
        descending), add_vals, cut_vals (per cube index, input order), and optionally the full
        probability vector / ranking.  Cubes of up to GRAPH_MAX_IDS distinct cards replay the
        captured request graph (one launch, one D2H); larger ones run the same kernels directly.
        With a `pool` (a CardPool) the additions are the pool's cards alone and the request takes
        the batched path, whose rows are bit-identical to this one; want_order with a pool raises."""
        if pool is not None:
            if want_order:
                raise ValueError('want_order is not available with a pool')
            return self.recommend_many([cube_indices], amount, want_probs=want_probs, pool=pool)[0]
        ci = np.asarray(cube_indices, np.int64)
        uniq = np.unique(ci).astype(np.int32)
        n = len(uniq)
        amount = int(amount)
        want = min(max(amount, 1), self.V - n)
        words = 1 + 2 * want + n
        with self.lock:
            req = self._req_np
            req[0] = n
            req[1] = amount
            req[2:2 + n] = uniq
            if n <= self.cap:
                L.call('cc_recommend_graph_run', self._graph_handle(), L.ptr(self.pin_res), words)
            else:
                with torch.cuda.stream(self.stream):
                    self.req_dev[:2 + n].copy_(self.pin_req[:2 + n], non_blocking=True)
                    L.call('cc_recommend_fp32', L.ptr(self.params), self.V, self.d, L.ptr(self.req_dev), n,
                           L.ptr(self.ws), L.ptr(self.probs_dev), L.ptr(self.res_dev), L.stream_ptr(self.stream))
                    self.pin_res[:words].copy_(self.res_dev[:words], non_blocking=True)
                self.stream.synchronize()
            r = self._res_np
            k = int(r[0])
            cut = r[1 + 2 * want:1 + 2 * want + n].view(np.float32)
            out = {
                'additions': r[1:1 + k].copy(),
                'add_vals': r[1 + want:1 + want + k].view(np.float32).copy(),
                'cut_vals': cut[np.searchsorted(uniq, ci)].copy() if n else np.zeros(0, np.float32),
            }
            probs = order = None
            if want_probs or want_order:
                probs = self.probs_dev.clone()   # the graph ran on its own stream and was waited for
            if want_order:
                order = self._full_order(probs, uniq, amount)
        if want_probs:
            out['probs'] = probs.cpu().numpy()
        if want_order:
            out['order'] = order
        return out

    # ------------------------------------------------------------------ many cubes per call
    def recommend_many(self, cubes, amount, want_probs=False, rows_per_launch=512, pool=None):
        """`recommend` for every cube of `cubes`, bit for bit, in launches of up to
        rows_per_launch rows (cc_recommend_batch_fp32: one pass over the output layer per row
        tile, one ranking workgroup per row).  Returns a list of dicts with the keys and dtypes of
        `recommend`: additions, add_vals, cut_vals (input order, duplicates kept), probs on
        request.  An id outside [0, V) raises ValueError before anything is launched.  Amounts
        above cc_recommend_batch_max_amount() take cc_recommend_batch_rank_fp32 (one sorting
        workgroup per row, result rows of min(amount, V) entries): its launches are capped by
        rank_rows_per_launch, and their results pass through two pinned staging buffers that the
        Recommender keeps.

        pool: None, one CardPool (card_pool) for every row, or a sequence of one CardPool or None
        per cube.  A row with a pool gets, as additions, the first max(amount, 1) members of
        pool minus cube in the row's unpooled ranking, every value bit for bit the unpooled
        call's (cc_recommend_batch_pool_fp32 / cc_recommend_batch_rank_pool_fp32); cut_vals and
        probs do not depend on the pool, nor does the choice of path.  A pool built for another V
        or a sequence of another length raises ValueError before anything is launched."""
        amount = int(amount)
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        R = len(inputs)
        pools, pool_of_row = resolve_pools(pool, R, self.V)
        if R == 0:
            return []
        check_card_ids(inputs, self.V)
        V, d, dev = self.V, self.d, self.dev
        rank = amount > int(L.lib().cc_recommend_batch_max_amount())
        stem = 'cc_recommend_batch_rank' if rank else 'cc_recommend_batch'
        if pools is not None:
            stem += '_pool'
        entry, ws_size = stem + '_fp32', getattr(L.lib(), stem + '_ws_size')
        if rank:
            A = min(max(amount, 1), V)
            rows_per_launch = rank_rows_per_launch(V, A, rows_per_launch, want_probs=want_probs)
        else:
            A = max(amount, 1)
        stage = self._rank_pins
        out = []

        def launch(r0, r1, turn):
            """Pack rows r0..r1, queue their launch and the copies of its results to pinned
            memory (fresh on the select path, the kept staging set of the turn's parity on the
            ranking path); no waiting."""
            row_ptr, idx, max_n, _, slot = pack_cubes(inputs[r0:r1], V)
            Rc, nnz = r1 - r0, len(idx)
            ws = self._batch_ws.get(ws_size(V, d, Rc, max_n), dev)
            rp_d, ix_d = upload(row_ptr, dev), upload(idx, dev)
            ints = torch.empty(Rc * (1 + A), device=dev, dtype=torch.int32)      # n_add, additions
            flts = torch.empty(Rc * A + max(nnz, 1), device=dev, dtype=torch.float32)  # add_vals, cuts
            probs = torch.empty(Rc, V, device=dev, dtype=torch.float32) if want_probs else None
            por_d = upload(pool_of_row[r0:r1], dev) if pools is not None else None
            L.call(entry, L.ptr(self.params), V, d, Rc, L.ptr(rp_d), L.ptr(ix_d), max_n,
                   amount, L.ptr(ws), L.ptr(ints), L.ptr(ints[Rc:]), L.ptr(flts),
                   L.ptr(flts[Rc * A:]), L.ptr(probs), *self._pool_args(table, por_d), L.stream_ptr(self.stream))
            host = [stage.kept(t, (turn & 1, i)) if rank else stage.fresh(t)
                    for i, t in enumerate((ints, flts, probs) if want_probs else (ints, flts))]
            return (nnz, slot, host), mark(self.stream)

        def collect(r0, r1, payload):
            nnz, slot, host = payload
            Rc = r1 - r0
            ints, flts = host[0].numpy().copy(), host[1].numpy().copy()   # out of the pinned staging
            nadd, adds, addv = ints[:Rc].tolist(), ints[Rc:].reshape(Rc, A), flts[:Rc * A].reshape(Rc, A)
            cuts = cuts_in_input_order(flts[Rc * A:Rc * A + nnz], slot, inputs[r0:r1])
            for r in range(Rc):
                k = nadd[r]
                o = {'additions': adds[r, :k], 'add_vals': addv[r, :k], 'cut_vals': cuts[r]}
                if want_probs:
                    o['probs'] = host[2][r].numpy().copy()
                out.append(o)

        with self.lock, torch.cuda.stream(self.stream):
            table = self._pool_table(pools) if pools is not None else None
            pipelined(row_spans(R, rows_per_launch), launch, collect)
        return out

    # ------------------------------------------------------------------ held-out evaluation
    def target_ranks(self, cubes, targets, cutoffs=(), rows_per_launch=512, pool=None):
        """Where the cards of targets[r] land in the ranking `recommend_many(cubes, <all>)` gives
        cube r, without ranking anything (cc_recommend_batch_target_ranks_fp32: the batched
        forward, then one counting workgroup per row; nothing of size R x V comes back).

        Returns (ranks, vals, hits): per cube an int32 array of 0-based positions in `additions`
        and a float32 array of the targets' probabilities, both in the caller's target order
        (duplicates kept); hits is None without cutoffs, else the device-side counters as a
        uint64 array [len(cutoffs) + 2]: targets with rank < cutoffs[k] for each k, then the
        targets counted, then the cubes whose best target has rank < cutoffs[0].  Up to 8
        cutoffs.  An id outside [0, V) in either list, or a target that is also in its cube,
        raises ValueError before anything is launched.

        pool (as for recommend_many): a row with a pool ranks its targets among the pool's cards
        outside the cube alone, the positions in the pooled `additions`
        (cc_recommend_batch_target_ranks_pool_fp32); a target outside its row's pool raises
        ValueError naming the cube and the card, as do a pool built for another V and a sequence
        of another length, all before anything is launched."""
        cutoffs = [int(k) for k in cutoffs]
        if len(cutoffs) > 8:
            raise ValueError('at most 8 cutoffs')
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        R = len(inputs)
        V, d = self.V, self.d
        pools, pool_of_row = resolve_pools(pool, R, V)
        check_card_ids(inputs, V)
        tgt_ptr, tgt = pack_targets(targets, inputs, V)
        if pools is not None:
            check_targets_in_pools(targets, pools, pool_of_row)
        if R == 0:
            return [], [], (np.zeros(len(cutoffs) + 2, np.uint64) if cutoffs else None)
        dev = self.dev
        stem = 'cc_recommend_batch_target_ranks' + ('_pool' if pools is not None else '')
        entry, ws_size = stem + '_fp32', getattr(L.lib(), stem + '_ws_size')

        def call(s):
            por_d = upload(pool_of_row[s.r0:s.r1], dev) if pools is not None else None
            ws = self._batch_ws.get(ws_size(V, d, s.Rc, s.max_n), dev)
            L.call(entry, L.ptr(self.params), V, d, s.Rc, L.ptr(s.rp), L.ptr(s.ix), s.max_n, L.ptr(s.tp),
                   L.ptr(s.tg), L.ptr(s.cut), s.nk, L.ptr(ws), L.ptr(s.rk), L.ptr(s.tv), L.ptr(s.hits),
                   L.ptr(s.cuts), None, *self._pool_args(table, por_d), L.stream_ptr(self.stream))

        with self.lock, torch.cuda.stream(self.stream):
            table = self._pool_table(pools) if pools is not None else None
            return target_ranks_rows(pack_cubes, inputs, V, tgt_ptr, tgt, cutoffs, rows_per_launch, dev,
                                     self.stream, self._rank_pins, torch.float32, call)

    # ------------------------------------------------------------------ validation loss
    def reconstruction_loss(self, cubes, targets=None, rows_per_launch=512):
        """The reconstruction output's loss of every cube, reduced per row on the device
        (cc_recommend_batch_loss_fp32: the batched forward of `recommend_many`, then the output
        tile with a loss epilogue; nothing of size R x V is written or copied back).

        Returns (row_loss float64 [R], row_pred int32 [R]): row r's binary cross-entropy of the
        logits of cubes[r] against the multi-hot row of targets[r] (mean over the V cards, fp64
        terms from the fp32 logits, summed in a fixed order: a row's bits do not depend on R or
        on the launch it falls into), and the first index of its largest probability (Keras'
        categorical accuracy compares it with the first target).  targets=None means the cubes
        themselves.  Duplicates collapse in both lists; an id outside [0, V) in either raises
        ValueError before anything is launched."""
        inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
        R = len(inputs)
        V, d = self.V, self.d
        check_card_ids(inputs, V)
        if targets is None:
            tgts = inputs
        else:
            tgts = [np.asarray(t, np.int64).reshape(-1) for t in targets]
            if len(tgts) != R:
                raise ValueError(f'{len(tgts)} target lists for {R} cubes')
            check_card_ids(tgts, V)
        row_loss, row_pred = np.zeros(R, np.float64), np.zeros(R, np.int32)
        if R == 0:
            return row_loss, row_pred
        dev, stage = self.dev, self._rank_pins

        def launch(r0, r1, turn):
            """Pack rows r0..r1, queue their launch and the copies of its results to pinned
            memory; no waiting."""
            row_ptr, idx, max_n, _, _ = pack_cubes(inputs[r0:r1], V)
            Rc = r1 - r0
            ws = self._batch_ws.get(L.lib().cc_recommend_batch_loss_ws_size(V, d, Rc, max_n), dev)
            tp_d, tg_d = rp_d, ix_d = upload(row_ptr, dev), upload(idx, dev)
            if targets is not None:
                tgt_ptr, tgt = pack_cubes(tgts[r0:r1], V)[:2]
                tp_d, tg_d = upload(tgt_ptr, dev), upload(tgt, dev)
            loss = torch.empty(Rc, device=dev, dtype=torch.float64)
            pred = torch.empty(Rc, device=dev, dtype=torch.int32)
            L.call('cc_recommend_batch_loss_fp32', L.ptr(self.params), V, d, Rc, L.ptr(rp_d), L.ptr(ix_d), max_n,
                   L.ptr(tp_d), L.ptr(tg_d), L.ptr(ws), L.ptr(loss), L.ptr(pred), L.stream_ptr(self.stream))
            return (stage.fresh(loss), stage.fresh(pred)), mark(self.stream)

        def collect(r0, r1, host):
            row_loss[r0:r1] = host[0].numpy()
            row_pred[r0:r1] = host[1].numpy()

        with self.lock, torch.cuda.stream(self.stream):
            pipelined(row_spans(R, rows_per_launch), launch, collect)
        return row_loss, row_pred

    # ------------------------------------------------------------------ leave-one-out scores
    def leave_one_out(self, cubes, targets=None, rows_per_launch=4096):
        """p(card | cube without c) for every card c of every cube (cc_leave_one_out_fp32): each
        value is, bit for bit, what `recommend_many` gives for the cube with c taken out, but the
        E1 chunk sums are shared between a cube's rows and the output layer runs at the wanted
        cards only.  Launches hold up to rows_per_launch derived rows (a cube of n distinct cards
        has n + 1); a larger cube is sliced by positions.  Returns one dict per cube.

        targets=None: loo_vals, p(c | cube without c), and cut_vals, p(c | cube) as
        `recommend_many` returns it; both float32 [m] in the cube's input order, duplicated ids
        repeating their value.
        targets: one list of card ids per cube, or one flat list for every cube; base float32 [T]
        is p(t | cube) and without float32 [m, T] is p(t | cube without the card of input entry
        i), in the order given.  A target may be a cube card and may be the card left out.  More
        results than the staging budget holds are split by targets as well as by rows.
        An id outside [0, V) in either argument raises ValueError before anything is launched."""
        from .leaveoneout import leave_one_out
        return leave_one_out(self, cubes, targets, rows_per_launch)

    # ------------------------------------------------------------------ greedy completion
    def complete_many(self, cubes, sizes, per_step=1, pool=None, rows_per_launch=512):
        """Fill every cube up to its size (cc_complete_fp32), bit for bit this loop per cube:
        S = its sorted distinct ids; while len(S) < size: r = recommend(S, per_step, pool=pool);
        take = r.additions[:size - len(S)]; stop if empty; S = sorted(S + take).  All passes of a
        launch run on the device with no host round trip; launches hold up to rows_per_launch
        cubes.  per_step=1 is exact greedy completion; a larger per_step (up to
        cc_complete_max_per_step()) lets the top per_step cards join per forward pass.

        sizes: one int for every cube or one per cube; a cube at or above its size gets nothing.
        pool: as for recommend_many; a row ends early when its candidates run out.
        Returns a list of {'added': int32 [k], 'added_vals': float32 [k]}: the cards in the order
        they were picked and the probability each had in the pass that picked it.  The caller's
        lists are not modified.  An id outside [0, V), a pool built for another V or another
        number of sizes or pools raises ValueError before anything is launched."""
        from .complete import complete_many
        return complete_many(self, cubes, sizes, per_step, pool, rows_per_launch)

    def complete(self, cube_indices, size, per_step=1, pool=None):
        """`complete_many` for one cube: {'added', 'added_vals'}."""
        return self.complete_many([cube_indices], size, per_step=per_step, pool=pool)[0]

    # ------------------------------------------------------------------ diverse recommendations
    def recommend_diverse_many(self, cubes, amount, trade=0.7, candidates=None, pool=None, emb=None,
                               rows_per_launch=512):
        """`recommend_many` re-ranked for diversity on the device (cc_recommend_diverse_fp32):
        greedy maximal marginal relevance over every cube's first `candidates` additions.  With
        c, p the additions and add_vals of recommend_many(cube, candidates, pool=pool), lam =
        np.float32(trade), mu = 1 - lam and red[j] = 0, pick number t is the untaken position j
        with the greatest (lam * p[j]) - (mu * red[j]) (fp32, every operation rounded; equal scores:
        the smaller j); then red[j] = max(red[j], sim(c[j], c[pick])) for every untaken j, sim the
        cosine of the cards' rows of `emb`, bit for bit the negated distance of similar_many.
        min(max(amount, 1), len(c)) cards are picked.  trade=1 is recommend_many(cubes, amount).

        candidates: None means min(cc_recommend_diverse_max_candidates(), max(4 * amount, 64)).
        emb: a [V, K] float32 table (tensor or array); None means similarity.card_embeddings.
        pool: as for recommend_many.
        Returns a list of dicts: additions int32, add_vals float32 (the bits of recommend_many),
        redundancy float32 (red[pick] when picked), base_rank int32 (the position j), all in pick
        order, and cut_vals as recommend_many returns them.  A trade outside [0, 1], candidates
        outside [1, cc_recommend_diverse_max_candidates()], a table that is not [V, K] or too wide
        for that many candidates, an id outside [0, V) and a wrong pool raise ValueError before
        anything is launched."""
        from .diverse import recommend_diverse_many
        return recommend_diverse_many(self, cubes, amount, trade, candidates, pool, emb, rows_per_launch)

    def recommend_diverse(self, cube_indices, amount, trade=0.7, candidates=None, pool=None, emb=None):
        """`recommend_diverse_many` for one cube."""
        return self.recommend_diverse_many([cube_indices], amount, trade=trade, candidates=candidates, pool=pool,
                                           emb=emb)[0]

    def _full_order(self, probs, uniq, amount):
        """The complete ranking (cc_topn with `order`; tests and tools only)."""
        V, dev = self.V, self.dev
        n = len(uniq)
        want = min(max(amount, 1), V)
        ci = torch.from_numpy(uniq if n else np.zeros(1, np.int32)).to(dev)
        adds = torch.zeros(want, device=dev, dtype=torch.int32)
        addv = torch.zeros(want, device=dev)
        cutv = torch.zeros(max(n, 1), device=dev)
        nadd = torch.zeros(1, device=dev, dtype=torch.int32)
        order = torch.zeros(V, device=dev, dtype=torch.int32)
        ws = torch.zeros(ws_elems(L.lib().cc_topn_workspace_size(V)), device=dev, dtype=torch.int32)
        L.call('cc_topn', L.ptr(probs), V, L.ptr(ci), n, amount, L.ptr(adds), L.ptr(nadd), L.ptr(addv),
               L.ptr(cutv), L.ptr(order), L.ptr(ws), L.stream_ptr())
        torch.cuda.synchronize()
        return order.cpu().numpy()
