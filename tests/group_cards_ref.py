"""The numpy restatement of the archetype card profiles (include/ccrec.h): all
integers.  count[g][v] = cubes of label g holding card v; size[g] = cubes of label g; total[v] = sum
over g of count[g][v]; N = sum of size.  Keys (a = count[g][v], t = total[v], s = size[g]):
rate a, lift a N - t s, avoid t s - a N; a card is a candidate when a >= max(min_count, 1) (avoid:
t >= max(min_count, 1)); a group's list is its candidates by key descending, equal keys lower card
first; found = min(m, candidates), 0 for a group of size 0."""
import numpy as np

KINDS = ('rate', 'lift', 'avoid')
KEY_OFFSET, CARD_BITS = 1 << 45, 18


def counts(row_ptr, idx, label, V, G):
    """(count uint32 [G][V], size int32 [G], total uint32 [V]) of the CSR's cubes under label."""
    row_ptr, label = np.asarray(row_ptr, np.int64), np.asarray(label, np.int64)
    lens = np.diff(row_ptr)
    lab_of_entry = np.repeat(label, lens)
    ids = np.asarray(idx, np.int64)[row_ptr[0]:row_ptr[-1]]
    keep = lab_of_entry >= 0
    count = np.bincount(lab_of_entry[keep] * V + ids[keep], minlength=G * V).reshape(G, V)
    size = np.bincount(label[label >= 0], minlength=G)
    return count.astype(np.uint32), size.astype(np.int32), count.sum(0).astype(np.uint32)


def keys(count, size, total, kind):
    """int64 [G][V]"""
    a, t = np.asarray(count, np.int64), np.asarray(total, np.int64)[None, :]
    s = np.asarray(size, np.int64)[:, None]
    N = int(np.asarray(size, np.int64).sum())
    return a + 0 * t if kind == 'rate' else a * N - t * s if kind == 'lift' else t * s - a * N


def top(count, size, total, kind, min_count, m):
    """(cards int32 [G][m], card_count uint32 [G][m], found int32 [G])"""
    count, total = np.asarray(count, np.int64), np.asarray(total, np.int64)
    G, V = count.shape
    k = keys(count, size, total, kind)
    need = max(int(min_count), 1)
    cards, ccnt = np.full((G, m), -1, np.int32), np.zeros((G, m), np.uint32)
    found = np.zeros(G, np.int32)
    for g in range(G):
        if size[g] <= 0:
            continue
        cand = np.flatnonzero((total if kind == 'avoid' else count[g]) >= need)
        order = cand[np.lexsort((cand, -k[g, cand]))][:m]
        found[g] = len(order)
        cards[g, :len(order)] = order
        ccnt[g, :len(order)] = count[g, order]
    return cards, ccnt, found


def composite(k, card):
    """The 64-bit composite of the select, as a Python int: ascending composites are the list."""
    return ((KEY_OFFSET - int(k)) << CARD_BITS) | int(card)


def csr(cubes):
    """(row_ptr int32 [R + 1], idx int32) of sorted distinct id lists."""
    lens = [len(c) for c in cubes]
    row_ptr = np.zeros(len(cubes) + 1, np.int32)
    row_ptr[1:] = np.cumsum(lens)
    idx = np.concatenate([np.asarray(c, np.int32) for c in cubes]) if len(cubes) and row_ptr[-1] else \
        np.zeros(0, np.int32)
    return row_ptr, idx.astype(np.int32)


def make_cubes(R, V, seed, mean=12):
    """R cubes over V cards: popularity-skewed sorted distinct ids, row lengths that put the row
    starts at every offset mod 4; cube 0 empty, cube 1 one card, cube 2 every card when V <= 300."""
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(1.0 / (1.0 + rng.permutation(V)))
    cdf /= cdf[-1]
    draws = rng.integers(0, 2 * mean + 1, R)
    cubes = []
    for r in range(R):          # draws with replacement, the distinct ones kept
        ids = np.unique(np.minimum(np.searchsorted(cdf, rng.random(int(draws[r]))), V - 1))
        if r == 0:
            ids = ids[:0]
        elif r == 1:
            ids = np.array([V // 2])
        elif r == 2 and V <= 300:
            ids = np.arange(V)
        cubes.append(ids.astype(np.int32))
    return cubes


LABELLINGS = ('one', 'third-out', 'empty-groups', 'single', 'skewed')


def make_labels(kind, R, G, seed):
    rng = np.random.default_rng(seed)
    if kind == 'one':                      # all cubes in one group (the last)
        return np.full(R, G - 1, np.int32)
    lab = rng.integers(0, G, R).astype(np.int32)
    if kind == 'third-out':
        lab[rng.random(R) < 1 / 3] = -1
    elif kind == 'empty-groups':           # only every third group is used
        lab = (lab // 3 * 3).astype(np.int32)
    elif kind == 'single':                 # group 0 holds exactly one cube (where there are two groups)
        if G > 1 and R > 0:
            lab[lab == 0] = G - 1
            lab[R // 2] = 0
    elif kind == 'skewed':                 # 90 % of the cubes in one group
        lab[rng.random(R) < 0.9] = min(1, G - 1)
    return lab
