"""The definition of greedy completion as a host loop (a helper, not a test): over the pinned-order
CPU oracle, and over any callable `recommend(S, m, pool) -> (additions, add_vals)`.

    S = sorted distinct ids of cube
    while len(S) < size:
        take = recommend(S, m, pool).additions[: size - len(S)]
        if none: break
        added += take;  S = sorted(S + take)
"""
import numpy as np

from oracle import infer_ref


def complete_loop(recommend, cube, size, per_step=1, pool=None):
    """The loop over `recommend`.  Returns (added int32 [k], added_vals float32 [k], final sorted S)."""
    S = np.unique(np.asarray(cube, np.int64))
    added, vals = [], []
    while len(S) < size:
        adds, addv = recommend(S, per_step, pool)
        take = np.asarray(adds, np.int64)[:size - len(S)]
        if len(take) == 0:
            break
        added += take.tolist()
        vals += np.asarray(addv, np.float32)[:len(take)].tolist()
        S = np.sort(np.concatenate([S, take]))
    return np.asarray(added, np.int32), np.asarray(vals, np.float32), S


def oracle_recommend(P, V):
    """recommend(S, m, pool) over oracle.infer_ref: the first m members of pool minus S (pool: a
    bool [V] mask or None) in the ranking of recommend_probs."""
    def recommend(S, m, pool):
        p = infer_ref.recommend_probs(P, S)
        order = infer_ref.rank(p)
        free = np.ones(V, bool)
        free[S] = False
        if pool is not None:
            free &= pool
        take = order[free[order]][:max(int(m), 1)]
        return take, p[take]
    return recommend


def recommender_recommend(rec):
    """recommend(S, m, pool) over Recommender.recommend_many, one cube per call (pool: a CardPool
    or None)."""
    def recommend(S, m, pool):
        out = rec.recommend_many([S], m, pool=pool)[0]
        return out['additions'], out['add_vals']
    return recommend


def complete_many_loop(rec, cubes, sizes, per_step=1, pools=None):
    """The loop over Recommender.recommend_many with every unfinished cube in one call per pass
    (what a caller has to write without complete_many).  pools: one CardPool or None per cube, or
    None.  Returns [(added, added_vals, final S)]."""
    R = len(cubes)
    sizes = [int(sizes)] * R if np.ndim(sizes) == 0 else [int(s) for s in sizes]
    S = [np.unique(np.asarray(c, np.int64)) for c in cubes]
    added, vals = [[] for _ in range(R)], [[] for _ in range(R)]
    live = [r for r in range(R) if len(S[r]) < sizes[r]]
    while live:
        outs = rec.recommend_many([S[r] for r in live], per_step,
                                  pool=None if pools is None else [pools[r] for r in live])
        nxt = []
        for r, o in zip(live, outs):
            take = o['additions'].astype(np.int64)[:sizes[r] - len(S[r])]
            if len(take) == 0:
                continue
            added[r] += take.tolist()
            vals[r] += o['add_vals'][:len(take)].tolist()
            S[r] = np.sort(np.concatenate([S[r], take]))
            if len(S[r]) < sizes[r]:
                nxt.append(r)
        live = nxt
    return [(np.asarray(a, np.int32), np.asarray(v, np.float32), s) for a, v, s in zip(added, vals, S)]
