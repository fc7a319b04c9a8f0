"""Diverse recommendations: greedy maximal marginal relevance over every cube's first
`candidates` recommendations on the device (cc_recommend_diverse_fp32, csrc/diverse.hip).

A launch ranks its rows' candidates with the batched select chain and re-ranks each row in one
workgroup; the host packs the cubes, sizes the output pitch and unpacks the picks.  Everything but
`recommend_diverse_many` itself is pure host code."""
import numpy as np
import torch

from . import _lib as L
from .launches import mark, pipelined, row_spans, upload
from .recommender import check_card_ids, cuts_in_input_order, pack_cubes, resolve_pools

DEFAULT_TRADE = 0.7


def default_candidates(amount, max_candidates):
    """candidates=None: four candidates per wanted card, at least 64, at most the kernel's limit."""
    return min(int(max_candidates), max(4 * int(amount), 64))


def plan_call(amount, trade, candidates, max_candidates):
    """The call's scalars as cc_recommend_diverse_fp32 takes them -> (amount, lam, M, A): lam is
    `trade` as np.float32, M the candidates per row, A = min(max(amount, 1), M) the output pitch
    (no row picks more).  Raises ValueError for a trade outside [0, 1] (NaN included) and for
    candidates outside [1, max_candidates]."""
    amount = int(amount)
    lam = np.float32(trade)
    if not (np.float32(0) <= lam <= np.float32(1)):
        raise ValueError(f'trade is {trade}: a number in [0, 1]')
    M = default_candidates(amount, max_candidates) if candidates is None else int(candidates)
    if M < 1:
        raise ValueError(f'candidates is {M}: at least 1')
    if M > int(max_candidates):
        raise ValueError(f'candidates is {M}: above cc_recommend_diverse_max_candidates() = {int(max_candidates)}')
    return amount, lam, M, min(max(amount, 1), M)


def k_pad(K):
    """K rounded up to the kernel's k stage of 32 (cosine::k_pad)."""
    return -(-max(int(K), 1) // 32) * 32


def check_table(shape, V, M, max_candidates):
    """ValueError unless an embedding table of `shape` is [V, K] with K >= 1 and M candidates of it
    fit the kernel's LDS tile: k_pad(K) * (M | 1) <= 64 * (max_candidates | 1)."""
    if len(shape) != 2 or int(shape[0]) != int(V) or int(shape[1]) < 1:
        raise ValueError(f'emb has shape {tuple(shape)}: [{int(V)}, K] with K >= 1')
    K = int(shape[1])
    if k_pad(K) * (int(M) | 1) > 64 * (int(max_candidates) | 1):
        fit = (64 * (int(max_candidates) | 1)) // k_pad(K)
        raise ValueError(f'{int(M)} candidates of {K} floats do not fit the LDS tile: at most {fit - 1 + (fit & 1)}')
    return K


def recommend_diverse_many(rec, cubes, amount, trade=DEFAULT_TRADE, candidates=None, pool=None, emb=None,
                           rows_per_launch=512):
    """The body of Recommender.recommend_diverse_many (documented there)."""
    V, d, dev = rec.V, rec.d, rec.dev
    lib = L.lib()
    cap = int(lib.cc_recommend_diverse_max_candidates())
    amount, lam, M, A = plan_call(amount, trade, candidates, cap)
    inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
    R = len(inputs)
    pools, pool_of_row = resolve_pools(pool, R, V)
    check_card_ids(inputs, V)
    if emb is not None:
        K = check_table(tuple(emb.shape), V, M, cap)
    if R == 0:
        return []
    if emb is None:
        from .similarity import card_embeddings
        emb = card_embeddings(rec)
        K = check_table(tuple(emb.shape), V, M, cap)
    if not torch.is_tensor(emb):
        emb = torch.from_numpy(np.ascontiguousarray(emb, np.float32))
    emb = emb.to(dev, torch.float32).contiguous()
    out = []

    def launch(r0, r1, turn):
        row_ptr, idx, max_n, _, slot = pack_cubes(inputs[r0:r1], V)
        Rc, nnz = r1 - r0, len(idx)
        ws = rec._batch_ws.get(lib.cc_recommend_diverse_ws_size(V, d, Rc, max_n, M, K), dev)
        rp_d, ix_d = upload(row_ptr, dev), upload(idx, dev)
        ints = torch.empty(Rc * (1 + 2 * A), device=dev, dtype=torch.int32)      # n_add, additions, base_rank
        flts = torch.empty(2 * Rc * A + max(nnz, 1), device=dev, dtype=torch.float32)   # add_vals, redundancy, cuts
        por_d = upload(pool_of_row[r0:r1], dev) if pools is not None else None
        pool_args = rec._pool_args(table, por_d, none=(None, 0, None))
        L.call('cc_recommend_diverse_fp32', L.ptr(rec.params), V, d, Rc, L.ptr(rp_d), L.ptr(ix_d), max_n, amount, M,
               float(lam), L.ptr(emb), K, *pool_args, A, L.ptr(ints), L.ptr(ints[Rc:]), L.ptr(flts),
               L.ptr(flts[Rc * A:]), L.ptr(ints[Rc * (1 + A):]), L.ptr(flts[2 * Rc * A:]), L.ptr(ws),
               ws.numel() * 4, L.stream_ptr(rec.stream))
        return (nnz, slot, rec._rank_pins.fresh(ints).numpy(), rec._rank_pins.fresh(flts).numpy()), mark(rec.stream)

    def collect(r0, r1, payload):
        nnz, slot, ints, flts = payload
        Rc = r1 - r0
        nadd = ints[:Rc].tolist()
        adds, rank = ints[Rc:Rc * (1 + A)].reshape(Rc, A), ints[Rc * (1 + A):].reshape(Rc, A)
        addv, red = flts[:Rc * A].reshape(Rc, A), flts[Rc * A:2 * Rc * A].reshape(Rc, A)
        cuts = cuts_in_input_order(flts[2 * Rc * A:2 * Rc * A + nnz], slot, inputs[r0:r1])
        for r in range(Rc):
            k = nadd[r]
            out.append({'additions': adds[r, :k].copy(), 'add_vals': addv[r, :k].copy(),
                        'redundancy': red[r, :k].copy(), 'base_rank': rank[r, :k].copy(), 'cut_vals': cuts[r]})

    with rec.lock, torch.cuda.stream(rec.stream):
        table = rec._pool_table(pools) if pools is not None else None
        pipelined(row_spans(R, rows_per_launch), launch, collect)
    return out
