"""Card audience — CPU reference over oracle/infer_ref.py (test infrastructure only).

h3 of a cube is encode32 and the three decoder dense32 layers; the probabilities of the asked
cards are dense32(h3, Wo[:, cards], bo[cards], relu=False) and det_sigmoid32.  Rows are batched
(dense32_rows): the arithmetic is element-wise per row, k in order, so a row's bits are dense32's.
Ranking per card: descending p, equal p lower cube id first, ids[np.lexsort((ids, -p))] over the
candidates (the cubes that do not hold the card, or every cube with include_members)."""
import numpy as np

from oracle import infer_ref
from oracle.detmath import det_sigmoid32

WO, BO = 'decoder/reconstruct/kernel', 'decoder/reconstruct/bias'


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dense32_rows(H, Wk, b, relu=True):
    """infer_ref.dense32 for the rows of H [R, K] at once: the same operations in the same order."""
    H, Wk = np.asarray(H, np.float32), np.asarray(Wk, np.float32)
    K = Wk.shape[0]
    total = np.zeros((H.shape[0], Wk.shape[1]), np.float32)
    for k0 in range(0, K, infer_ref.DOT_CHUNK):
        part = np.zeros_like(total)
        for k in range(k0, min(K, k0 + infer_ref.DOT_CHUNK)):
            part = (part + (H[:, k:k + 1] * Wk[k][None, :]).astype(np.float32)).astype(np.float32)
        total = (total + part).astype(np.float32)
    out = (total + np.asarray(b, np.float32)[None, :]).astype(np.float32)
    return np.where(out > 0, out, np.float32(0)).astype(np.float32) if relu else out


def h3_rows(P, cubes):
    """The decoder's last hidden row of every cube: [R, d] fp32."""
    d = P['encoder/encoded_1/kernel'].shape[1]
    if not len(cubes):
        return np.zeros((0, d), np.float32)
    h = np.stack([infer_ref.gather_e1(P['encoder/encoded_1/kernel'], P['encoder/encoded_1/bias'], c) for c in cubes])
    for nm in infer_ref.TOWER:
        h = dense32_rows(h, P[nm + '/kernel'], P[nm + '/bias'])
    return h


def probs_at(P, h3, cards):
    """p [R, T] of the asked cards (any order, duplicates allowed)."""
    cards = np.asarray(cards, np.int64).reshape(-1)
    z = dense32_rows(h3, P[WO][:, cards], P[BO][cards], relu=False)
    return det_sigmoid32(z)


def membership(cubes, V):
    m = np.zeros((len(cubes), V), bool)
    for r, c in enumerate(cubes):
        m[r, np.asarray(c, np.int64).reshape(-1)] = True
    return m


class Ref:
    """A corpus on the CPU: every card's probability for every cube, once."""

    def __init__(self, P, cubes, V):
        self.V, self.N = V, len(cubes)
        self.h3 = h3_rows(P, cubes)
        self.p = probs_at(P, self.h3, np.arange(V))             # [N, V]
        self.member = membership(cubes, V)

    def expected(self, cards, k, include_members=False, threshold=0.5, N=None):
        """(cubes [T, n], probs [T, n], counts [T, 3]) over the first N cubes, n = min(k, N); a
        card outside [0, V) gives an empty row and zero counts."""
        N = self.N if N is None else N
        cards = np.asarray(cards, np.int64).reshape(-1)
        n = max(0, min(int(k), N))
        out_i = np.full((len(cards), n), -1, np.int32)
        out_p = np.zeros((len(cards), n), np.float32)
        counts = np.zeros((len(cards), 3), np.int32)
        thr = np.float32(threshold)
        ids = np.arange(N)
        for t, card in enumerate(cards.tolist()):
            if not 0 <= card < self.V:
                continue
            p, mem = self.p[:N, card], self.member[:N, card]
            cand = np.ones(N, bool) if include_members else ~mem
            ci, cp = ids[cand], p[cand]
            order = np.lexsort((ci, -cp))[:n]
            out_i[t, :len(order)] = ci[order]
            out_p[t, :len(order)] = cp[order]
            counts[t] = (mem.sum(), cand.sum(), (cp >= thr).sum())
        return out_i, out_p, counts
