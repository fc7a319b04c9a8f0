"""Held-out evaluation of the recommender: hide some of a cube's cards, show the model the rest,
and ask where the hidden cards land in its ranking.

Pure host code except the one call of Recommender.target_ranks, which returns every hidden card's
exact position in the ranking `recommend_many(visible, <all>)` would give, without ranking anything
(cc_recommend_batch_target_ranks_fp32).  The metrics are float64 functions of those integers.

evaluate_loss is the other held-out number, the training loss on cubes the model did not train on:
Recommender.reconstruction_loss (cc_recommend_batch_loss_fp32) reduces every row's binary
cross-entropy and argmax on the device, the host takes the means.
"""
import inspect

import numpy as np


def holdout_split(cubes, hide=0.2, min_visible=1, seed=0):
    """Split every cube into (visible, hidden) card lists -> two lists of int64 arrays, both
    sorted ascending.

    Duplicates in a cube are collapsed first.  `hide` below 1 is a fraction of the cube's n
    distinct cards, rounded down, with at least 1 hidden where n >= 2; an integer `hide` >= 1 is a
    count.  At least min_visible cards always stay visible (so a cube of min_visible cards or
    fewer hides nothing).  Deterministic from `seed` alone: one numpy.random.default_rng(seed),
    cubes in order, one draw per cube that hides anything."""
    if hide < 0:
        raise ValueError('hide must not be negative')
    as_count = hide >= 1
    if as_count and int(hide) != hide:
        raise ValueError('hide is a fraction below 1 or an integer count')
    rng = np.random.default_rng(seed)
    visible, hidden = [], []
    for c in cubes:
        u = np.unique(np.asarray(c, np.int64).reshape(-1))
        n = len(u)
        k = int(hide) if as_count else int(np.floor(hide * n))
        if not as_count and hide > 0 and n >= 2:
            k = max(k, 1)
        k = max(0, min(k, n - int(min_visible)))
        if k == 0:
            visible.append(u)
            hidden.append(np.zeros(0, np.int64))
            continue
        mask = np.zeros(n, bool)
        mask[rng.choice(n, k, replace=False)] = True
        visible.append(u[~mask])
        hidden.append(u[mask])
    return visible, hidden


def metrics_from_ranks(ranks, ks):
    """Ranking metrics from the hidden cards' 0-based ranks (one integer array per cube; a
    negative rank is not a target and is ignored) -> dict of float64 / int:

      recall@K   micro-averaged over targets: targets with rank < K / targets
      ndcg@K     per cube, binary relevance: sum over its targets with rank < K of
                 1 / log2(rank + 2), over the ideal sum_{i < min(K, hidden)} 1 / log2(i + 2);
                 mean over the cubes with at least one target
      hit_rate@K share of those cubes with at least one target of rank < K
      mrr        mean over those cubes of 1 / (best rank + 1)
      n_cubes    cubes with at least one target;  n_targets  targets counted

    A model cannot place two cards at one rank, so the ideal DCG is reachable only with distinct
    targets per cube (holdout_split gives those)."""
    ks = [int(k) for k in ks]
    rows = []
    for r in ranks:
        r = np.asarray(r, np.int64).reshape(-1)
        rows.append(r[r >= 0])
    rows = [r for r in rows if len(r)]
    n_cubes = len(rows)
    n_targets = int(sum(len(r) for r in rows))
    out = {}
    max_t = max((len(r) for r in rows), default=0)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(max_t, dtype=np.float64) + 2.0))])
    for K in ks:
        hits = sum(int(np.count_nonzero(r < K)) for r in rows)
        out[f'recall@{K}'] = hits / n_targets if n_targets else 0.0
        ndcg = [float(np.sum(1.0 / np.log2(r[r < K].astype(np.float64) + 2.0))) / ideal[min(K, len(r))]
                if K > 0 else 0.0 for r in rows]
        out[f'ndcg@{K}'] = float(np.mean(ndcg)) if n_cubes else 0.0
        out[f'hit_rate@{K}'] = float(np.mean([float(r.min() < K) for r in rows])) if n_cubes else 0.0
    out['mrr'] = float(np.mean([1.0 / (float(r.min()) + 1.0) for r in rows])) if n_cubes else 0.0
    out['n_cubes'] = n_cubes
    out['n_targets'] = n_targets
    return out


def evaluate_loss(model, cubes, targets=None, rows_per_launch=512):
    """The reconstruction output's loss and accuracy on `cubes` (clean inputs; targets=None means
    the cubes themselves) -> {'bce', 'output_1_accuracy', 'n_cubes'}: what Keras' model.evaluate
    reports for output 1.  `model` is a CC_Recommender or a Recommender; the per-row reduction
    runs on the device (Recommender.reconstruction_loss).

      bce                mean over the cubes of the row losses (float64 sum / R)
      output_1_accuracy  categorical accuracy: the share of rows whose most probable card (first
                         index on ties) is the row's first (lowest) target id, 0 for a row without
                         targets - tf.argmax of the multi-hot row"""
    rec = model.recommender() if hasattr(model, 'recommender') else model
    cubes = list(cubes)
    row_loss, row_pred = rec.reconstruction_loss(cubes, targets, rows_per_launch=rows_per_launch)
    R = len(cubes)
    if R == 0:
        return {'bce': 0.0, 'output_1_accuracy': 0.0, 'n_cubes': 0}
    first = np.zeros(R, np.int64)
    for r, t in enumerate(cubes if targets is None else targets):
        t = np.asarray(t, np.int64).reshape(-1)
        first[r] = t.min() if len(t) else 0
    hits = int(np.count_nonzero(np.asarray(row_pred, np.int64) == first))
    return {'bce': float(np.sum(np.asarray(row_loss, np.float64))) / R, 'output_1_accuracy': hits / R,
            'n_cubes': R}


def evaluate_holdout(model, cubes, ks=(10, 50, 100), hide=0.2, seed=0, min_visible=1, rows_per_launch=512,
                     pool=None):
    """holdout_split -> target_ranks -> metrics_from_ranks.  `model` is a CC_Recommender or a
    Recommender.  The device's own counters come back under 'hits' (uint64 list: targets with
    rank < K for each K, targets counted, cubes whose best target has rank < ks[0]).

    pool (one CardPool for every cube, or one CardPool or None per cube): a hidden card is ranked
    among the cards of its cube's pool alone, where the user could have picked it.  The split is
    the unpooled one; hidden cards outside their cube's pool are dropped on the host and counted
    under 'n_targets_outside_pool', the metrics are over the rest.  A model whose target_ranks
    takes no pool (GraphRecommender) raises ValueError."""
    rec = model.recommender() if hasattr(model, 'recommender') else model
    visible, hidden = holdout_split(cubes, hide=hide, min_visible=min_visible, seed=seed)
    if pool is None:
        ranks, _, hits = rec.target_ranks(visible, hidden, cutoffs=ks, rows_per_launch=rows_per_launch)
        out = metrics_from_ranks(ranks, ks)
    else:
        from .recommender import pools_per_row
        if 'pool' not in inspect.signature(rec.target_ranks).parameters:
            raise ValueError(f'{type(rec).__name__}.target_ranks takes no pool')
        kept = [h if p is None else h[p.contains(h)] for h, p in zip(hidden, pools_per_row(pool, len(hidden)))]
        ranks, _, hits = rec.target_ranks(visible, kept, cutoffs=ks, rows_per_launch=rows_per_launch, pool=pool)
        out = metrics_from_ranks(ranks, ks)
        out['n_targets_outside_pool'] = int(sum(len(h) - len(k) for h, k in zip(hidden, kept)))
    if hits is not None:
        out['hits'] = [int(h) for h in hits]
    return out
