"""The definition of the diverse re-ranking (greedy maximal marginal relevance) in
numpy float32, every operation rounded on its own (a helper, not a test).

    c, p  : the candidates and their probabilities, best first (recommend_many's additions, add_vals)
    sim   : the negated distance of oracle.similarity_ref.cosine_dists on the candidates' rows of emb
    lam = float32(trade); mu = 1 - lam; red[j] = +0
    pick t: the untaken j of greatest (lam * p[j]) - (mu * red[j]), equal scores the smallest j;
            then for every untaken j: s = sim(c[j], c[pick]); if s > red[j]: red[j] = s
"""
import numpy as np

from oracle import similarity_ref


def mmr(c, p, emb, amount, trade):
    """-> (ids int32 [picks], p float32, the redundancy charged float32, base rank int32), picks =
    min(max(amount, 1), len(c)), in pick order."""
    f = np.float32
    c = np.asarray(c, np.int64).reshape(-1)
    p = np.asarray(p, f).reshape(-1)
    cnt = len(c)
    picks = min(max(int(amount), 1), cnt)
    lam = f(trade)
    mu = f(f(1) - lam)
    rows = np.asarray(emb, f)[c]
    red = np.zeros(cnt, f)
    taken = np.zeros(cnt, bool)
    lp = (lam * p).astype(f)
    ids, vals, charged, rank = [], [], [], []
    for t in range(picks):
        score = (lp - (mu * red).astype(f)).astype(f)
        free = np.flatnonzero(~taken)
        j = int(free[np.argmax(score[free])])       # argmax: the first of the greatest values
        ids.append(c[j]), vals.append(p[j]), charged.append(red[j]), rank.append(j)
        taken[j] = True
        if t + 1 < picks:
            s = (-similarity_ref.cosine_dists(rows, j)).astype(f)
            up = ~taken & (s > red)
            red[up] = s[up]
    return np.asarray(ids, np.int32), np.asarray(vals, f), np.asarray(charged, f), np.asarray(rank, np.int32)


def host_loop(outs, emb, amount, trade):
    """mmr over the dicts recommend_many(cubes, candidates) returns: what a caller has to write
    without recommend_diverse_many."""
    return [mmr(o['additions'], o['add_vals'], emb, amount, trade) for o in outs]
