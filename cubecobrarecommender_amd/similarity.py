"""Card similarity (src/scripts/similarity.py:19-31) on the GPU: the encoder on
the identity (cc_infer_encode_fp32 on one-card rows, the same kernel as model.encoder) gives the
[V, 64] card embeddings, cached per model; cc_similar_cards scores every card against the query
with Keras CosineSimilarity and returns the N smallest distances (argsort order, ties -> lower
index first).  similar_many / similarity_table serve many query cards per call
(cc_similar_cards_batch: every card normalised once, the rows ranked on the device)."""
import threading

import numpy as np
import torch

from . import _lib as L
from .launches import Staging, Workspace, mark, pipelined, row_spans, upload


def card_embeddings(model):
    """model.encoder(I[V, V]) -> [V, 64] fp32 on the device (cached on the model object)."""
    rec = model.recommender() if hasattr(model, 'recommender') else model
    emb = getattr(rec, '_card_emb', None)
    if emb is None:
        emb = rec.encode_lists([[i] for i in range(rec.V)])
        rec._card_emb = emb
    return emb


SIM_NMAX = 4096   # cc_similar_cards' in-LDS selection limit (csrc/similarity.hip)


def similar(emb, idx, N):
    """(indices [N] int64, dists [N] float32) of the N cards closest to card idx (idx itself first
    unless another card ties at -1).  N <= 0 gives empty arrays (the reference's loop prints
    nothing); N is capped at V.  Up to SIM_NMAX the selection runs in cc_similar_cards' one-workgroup
    radix select; beyond it the same kernel's distance vector is fully sorted on the device
    (stable, ties -> lower index, as numpy's argsort(kind='stable'))."""
    emb = emb.contiguous()
    V, K = emb.shape
    N = min(int(N), V)
    if N <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    dev = emb.device
    ws = torch.empty(int(L.lib().cc_similar_ws_size(V)) // 8 + 1, device=dev, dtype=torch.int64)
    n_sel = min(N, SIM_NMAX)
    out_idx = torch.empty(n_sel, device=dev, dtype=torch.int32)
    out_d = torch.empty(n_sel, device=dev, dtype=torch.float32)
    dist_all = torch.empty(V, device=dev, dtype=torch.float32)
    L.call('cc_similar_cards', L.ptr(emb), V, K, int(idx), n_sel, L.ptr(out_idx), L.ptr(out_d),
           L.ptr(dist_all), L.ptr(ws), L.stream_ptr())
    if N > SIM_NMAX:
        order = torch.sort(dist_all, stable=True).indices[:N]
        out_idx, out_d = order, dist_all[order]
    torch.cuda.current_stream().synchronize()
    return out_idx.cpu().numpy().astype(np.int64), out_d.cpu().numpy()


def similar_cards(model, name, N, int_to_card, card_to_int):
    """similarity.py:19-31 for one card name: [(rank, name, dist)] for ranks 1..N."""
    emb = card_embeddings(model)
    idx, dists = similar(emb, card_to_int[name], N)
    return [(i + 1, int_to_card[int(j)], float(dv)) for i, (j, dv) in enumerate(zip(idx, dists))]


# ---------------------------------------------------------------------- many query cards per call
_ws_lock = threading.Lock()
_ws = {}          # device -> the batched entry's Workspace
_stage = Staging()


def _similar_rows(emb, queries, n, rows_per_launch, idx_dtype):
    """cc_similar_cards_batch on queries (int32, all inside [0, V)) in launches of up to
    rows_per_launch rows: (indices idx_dtype [Q, n], dists float32 [Q, n]).  A launch's results
    are copied to pinned memory behind it and unpacked while the next launch runs."""
    V, K = emb.shape
    Q, dev = len(queries), emb.device
    out_i, out_d = np.empty((Q, n), idx_dtype), np.empty((Q, n), np.float32)

    def launch(r0, r1, turn):
        Rc = r1 - r0
        ws = kept.get(L.lib().cc_similar_batch_ws_size(V, K, Rc, n), dev)
        q_d = upload(queries[r0:r1], dev)
        idx = torch.empty(Rc, n, device=dev, dtype=torch.int32)
        dist = torch.empty(Rc, n, device=dev, dtype=torch.float32)
        L.call('cc_similar_cards_batch', L.ptr(emb), V, K, Rc, L.ptr(q_d), n, L.ptr(ws), L.ptr(idx),
               L.ptr(dist), None, L.stream_ptr())
        return (_stage.fresh(idx), _stage.fresh(dist)), mark()

    def collect(r0, r1, host):
        out_i[r0:r1] = host[0].numpy()
        out_d[r0:r1] = host[1].numpy()

    with _ws_lock:        # one workspace per device: one caller at a time
        kept = _ws.setdefault(dev, Workspace())
        last = pipelined(row_spans(Q, rows_per_launch), launch, collect)
        torch.cuda.current_stream().synchronize()   # the workspace is free for the next caller's stream
        del last    # only now: freeing pinned memory records an event on the stream (16 us inside the wait)
    return out_i, out_d


def similar_many(emb, idxs, N, rows_per_launch=512):
    """`similar` for every card of idxs (duplicates allowed) through cc_similar_cards_batch:
    (indices int64 [Q, n], dists float32 [Q, n]) with n = min(N, V), every row the bits
    similar(emb, idx, N) returns, whatever batch or launch it falls into.  N <= 0 gives [Q, 0]
    arrays; an id outside [0, V) raises ValueError before anything is launched."""
    V, K = emb.shape
    q = np.asarray(idxs, np.int64).reshape(-1)
    bad = np.flatnonzero((q < 0) | (q >= V))
    if len(bad):
        raise ValueError(f'query {int(bad[0])}: card id {int(q[bad[0]])} outside [0, {V})')
    n = max(0, min(int(N), V))
    if n == 0 or len(q) == 0:
        return np.zeros((len(q), n), np.int64), np.zeros((len(q), n), np.float32)
    return _similar_rows(emb.contiguous(), q.astype(np.int32), n, rows_per_launch, np.int64)


def similar_cards_many(model, names, N, int_to_card, card_to_int):
    """`similar_cards` for every name of names, in one batched request: a list of
    [(rank, name, dist)] lists."""
    emb = card_embeddings(model)
    idx, dists = similar_many(emb, [card_to_int[name] for name in names], N)
    return [[(i + 1, int_to_card[int(j)], float(dv)) for i, (j, dv) in enumerate(zip(row, drow))]
            for row, drow in zip(idx, dists)]


def similarity_table(model_or_emb, N, rows_per_launch=512):
    """The N nearest cards of every card: (indices int32 [V, n], dists float32 [V, n]),
    n = min(N, V); row j is similar(emb, j, N).  Takes a model or its [V, K] embeddings."""
    emb = model_or_emb if torch.is_tensor(model_or_emb) else card_embeddings(model_or_emb)
    V = emb.shape[0]
    n = max(0, min(int(N), V))
    if n == 0:
        return np.zeros((V, 0), np.int32), np.zeros((V, 0), np.float32)
    return _similar_rows(emb.contiguous(), np.arange(V, dtype=np.int32), n, rows_per_launch, np.int32)
