"""cc_group_cards_count and cc_group_cards_top on the GPU by direct calls: every output equal to the
numpy reference (tests/group_cards_ref.py), exactly.  Workspaces are filled with junk, outputs too
(accumulate == 0 must zero them) with a guard word behind each.

The kernels' own edges:
  the LDS tile of cc_group_cards_tile() cards -> V in {1, 63, 65, 2000, tile - 1, tile, tile + 1, 2 tile + 5}
  1,024 cubes per label histogram, a wave per cube, the slices -> R in {0, 1, 255, 257, 5000}
  a thread per group of the plan                -> G in {1, 2, 65, max_groups}
  labellings: one group, a third unlabelled, empty groups, a one-cube group, 90 % in one group (at
  R = 5000 that group is cut into about 18 slices and flushes with atomics; the others store)
  cubes: an empty one, a one-card one, one with every card (V <= 300), row starts at every offset mod 4
Every case runs under path 1, 2 and 0, and as two accumulated spans [0, r), [r, R) for r in
{1, 256, R - 1}, the second span also under the other path."""
import ctypes as C

import numpy as np
import pytest

from tests import group_cards_ref as R
from tests.test_gpu_cube_cluster import JUNK_I, guarded, unguarded
from tests.test_gpu_cube_neighbours import JUNKS, junk_buffer, lib

pytestmark = pytest.mark.gpu

TILE, MAX_G = 22528, 1024          # asserted against the library in test_constants_are_the_librarys
KIND = {'rate': 0, 'lift': 1, 'avoid': 2}


def test_constants_are_the_librarys():
    assert int(lib().cc_group_cards_tile()) == TILE and int(lib().cc_group_cards_max_groups()) == MAX_G >= 1024


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset)


class Tables:
    """count [G][V], size [G], total [V] on the device, junk-filled and guarded."""

    def __init__(self, G, V):
        import torch
        self.G, self.V = G, V
        self.count, self.size, self.total = (guarded(n, torch.int32, JUNK_I) for n in (G * V, G, V))

    def host(self):
        return (unguarded(self.count).view(np.uint32).reshape(self.G, self.V), unguarded(self.size),
                unguarded(self.total).view(np.uint32))


class Case:
    def __init__(self, V, Rn, G, labelling, seed):
        import torch
        self.V, self.R, self.G = V, Rn, G
        self.cubes = R.make_cubes(Rn, V, seed)
        self.row_ptr, self.idx = R.csr(self.cubes)
        self.label = R.make_labels(labelling, Rn, G, seed + 1)
        up = lambda a: torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()    # noqa: E731
        self.rp_d, self.ix_d, self.lab_d = up(self.row_ptr), up(self.idx), up(self.label)
        self.want = R.counts(self.row_ptr, self.idx, self.label, V, G)

    def count(self, tables, r0, r1, accumulate, path, junk=JUNKS[0]):
        import torch
        from cubecobrarecommender_amd import _lib as L
        ws = junk_buffer(lib().cc_group_cards_ws_size(r1 - r0, self.V, self.G, 1), junk)
        rc = lib().cc_group_cards_count(ptr(self.rp_d, r0), ptr(self.ix_d), r1 - r0, self.V, ptr(self.lab_d, r0), self.G,
                                        accumulate, path, L.ptr(ws), L.ptr(tables.count), L.ptr(tables.size),
                                        L.ptr(tables.total), L.stream_ptr())
        assert rc == 0, lib().cc_last_error_string()
        torch.cuda.synchronize()

    def check(self, tables, what):
        got = tables.host()
        for name, g, w in zip(('count', 'size', 'total'), got, self.want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, int((g != w).sum()))


def run_top(count, size, total, kind, min_count, m, junk=JUNKS[0]):
    """A direct cc_group_cards_top call on host arrays: (cards, card_count, found)."""
    import torch
    from cubecobrarecommender_amd import _lib as L
    G, V = count.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
           for a in (count.astype(np.uint32), size.astype(np.int32), total.astype(np.uint32))]
    ws = junk_buffer(lib().cc_group_cards_ws_size(0, V, G, m), junk)
    cards, ccnt, found = guarded(G * m, torch.int32, JUNK_I), guarded(G * m, torch.int32, JUNK_I), \
        guarded(G, torch.int32, JUNK_I)
    rc = lib().cc_group_cards_top(L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), V, G, KIND[kind], min_count, m, L.ptr(ws),
                                  L.ptr(cards), L.ptr(ccnt), L.ptr(found), L.stream_ptr())
    assert rc == 0, lib().cc_last_error_string()
    torch.cuda.synchronize()
    return unguarded(cards).reshape(G, m), unguarded(ccnt).view(np.uint32).reshape(G, m), unguarded(found)


def check_top(count, size, total, kind, min_count, m):
    got = run_top(count, size, total, kind, min_count, m)
    want = R.top(count, size, total, kind, min_count, m)
    for name, g, w in zip(('cards', 'card_count', 'found'), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (kind, min_count, m, name, int((g != w).sum()))
    return want


def cases():
    out = []
    for i, V in enumerate((1, 63, 65, 2000, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)):     # every V
        out.append((V, 257, 2, R.LABELLINGS[1 + i % 4]))
    for V in (2000, TILE + 1, 2 * TILE + 5):                                               # several slices and tiles
        out.append((V, 5000, 65, 'skewed'))
    for i, Rn in enumerate((0, 1, 255, 257, 5000)):                                        # every R at every G
        for j, G in enumerate((1, 2, 65, MAX_G)):
            out.append((2000, Rn, G, R.LABELLINGS[(i + j) % 5]))
    for lab in R.LABELLINGS:                                                               # every labelling
        out.append((300, 5000, 65, lab))
        out.append((65, 257, MAX_G, lab))
    return out


@pytest.mark.parametrize('V,Rn,G,labelling', cases())
def test_counts_against_the_reference(V, Rn, G, labelling):
    case = Case(V, Rn, G, labelling, seed=V + 3 * Rn + G)
    for n, path in enumerate((1, 2, 0)):
        tables = Tables(G, V)
        case.count(tables, 0, Rn, 0, path, junk=JUNKS[n % 2])
        case.check(tables, f'path {path}')
    for r in sorted({r for r in (1, 256, Rn - 1) if 0 < r < Rn}):
        for first, second in ((1, 1), (2, 2), (1, 2), (2, 1), (0, 0)):
            tables = Tables(G, V)
            case.count(tables, 0, r, 0, first)
            case.count(tables, r, Rn, 1, second, junk=JUNKS[1])
            case.check(tables, f'spans at {r}, paths {first} {second}')
    if Rn:                                   # accumulating nothing changes nothing
        case.count(tables, 0, 0, 1, 0)
        case.check(tables, 'an empty span')
    count, size, total = case.want           # and the lists of these counts
    kind = R.KINDS[(V + Rn + G) % 3]
    check_top(count, size, total, kind, 1, 7)


def test_a_skewed_group_is_cut_into_slices_and_labels_of_every_kind_occur():
    """What the cases above are taken to exercise, in the reference's terms."""
    lab = R.make_labels('skewed', 5000, 65, 1)
    assert np.bincount(lab[lab >= 0]).max() > 4000
    assert (R.make_labels('third-out', 5000, 65, 1) == -1).sum() > 1000
    assert (np.bincount(R.make_labels('empty-groups', 5000, 65, 1), minlength=65) == 0).sum() > 30
    assert np.bincount(R.make_labels('single', 5000, 65, 1), minlength=65)[0] == 1
    starts = R.csr(R.make_cubes(257, 2000, 5))[0][:-1]
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}
    cubes = R.make_cubes(257, 65, 5)
    assert len(cubes[0]) == 0 and len(cubes[1]) == 1 and len(cubes[2]) == 65


# ------------------------------------------------------------------ cc_group_cards_top on synthetic arrays
def limit_arrays(seed):
    """G = 2, V = 300, N = 2^22: counts a from 0 to s, the ends included; totals their sums."""
    rng = np.random.default_rng(seed)
    V, N = 300, 1 << 22
    size = np.array([(1 << 21) + 12345, (1 << 21) - 12345], np.int64)
    count = np.stack([rng.integers(0, s + 1, V) for s in size])
    count[:, :4] = [[0, 1, 2, 3], [3, 2, 1, 0]]
    count[0, 4], count[1, 4] = size[0], 0
    count[0, 5], count[1, 5] = 0, size[1]
    count[:, 6] = size
    count[:, 7:11] = count[:, 11:15]                  # equal counts: equal keys of `rate`
    return count, size, count.sum(0)


@pytest.mark.parametrize('kind', R.KINDS)
def test_top_with_keys_at_the_limits(kind):
    count, size, total = limit_arrays(3)
    for m in (1, 7, 1024):                            # 1,024 is above the 300 cards
        for min_count in (1, 3, 1 << 30):
            want = check_top(count, size, total, kind, min_count, m)
            if min_count == 1 << 30:
                assert np.all(want[2] == 0) and np.all(want[0] == -1)
    assert check_top(count, size, total, kind, 0, 1024)[2].max() <= 300
    # one group holds every cube: s = N = 2^22, and arrays that are no counts of anything reach
    # |key| = 2^44 in both signs (a = s with t = 0, a = 0 with t = N)
    N = 1 << 22
    size1 = np.array([N, 0], np.int64)
    count1 = np.zeros((2, 300), np.int64)
    count1[0] = np.random.default_rng(5).integers(0, N + 1, 300)
    total1 = np.random.default_rng(6).integers(1, N + 1, 300)
    count1[0, :3], total1[:3] = [N, 0, N], [1, N, N]
    count1[1] = 7
    for m in (7, 1024):
        want = check_top(count1, size1, total1, kind, 1, m)
        assert want[2][1] == 0                        # the group of size 0


def test_top_with_equal_keys_lists_the_cards_ascending():
    V = 300
    count = np.full((2, V), 5, np.int64)
    size = np.array([9, 11], np.int64)
    for kind in R.KINDS:
        want = check_top(count, size, count.sum(0), kind, 1, 1024)
        assert want[2].tolist() == [V, V] and want[0][0, :V].tolist() == list(range(V))
    big = np.full((1, 2 * TILE + 5), 2, np.int64)     # and over more cards than one pass of the select holds
    want = check_top(big, np.array([2]), big.sum(0), 'lift', 1, 1024)
    assert want[0][0].tolist() == list(range(1024))


def test_bad_arguments_launch_nothing():
    import torch
    from cubecobrarecommender_amd import _lib as L
    case = Case(300, 257, 2, 'third-out', seed=1)
    tables = Tables(2, 300)
    ws = torch.zeros(int(lib().cc_group_cards_ws_size(257, 300, 2, 7)) // 4 + 64, device='cuda', dtype=torch.int32)

    def count(R_=257, V=300, G=2, accumulate=0, path=0, ws_off=0, label=case.lab_d):
        rc = lib().cc_group_cards_count(ptr(case.rp_d), ptr(case.ix_d), R_, V, None if label is None else ptr(label), G,
                                        accumulate, path, ptr(ws, ws_off), L.ptr(tables.count), L.ptr(tables.size),
                                        L.ptr(tables.total), L.stream_ptr())
        return rc, lib().cc_last_error_string()
    for kw in (dict(R_=-1), dict(R_=(1 << 22) + 1), dict(V=0), dict(V=(1 << 18) + 1), dict(G=0), dict(G=MAX_G + 1),
               dict(accumulate=2), dict(path=3), dict(path=-1), dict(ws_off=2), dict(label=None)):
        rc, msg = count(**kw)
        assert rc == -1 and b'cc_group_cards_count' in msg, kw
    out = guarded(2 * 7, torch.int32, JUNK_I)

    def top(V=300, G=2, kind=1, min_count=1, m=7, ws_off=0):
        rc = lib().cc_group_cards_top(L.ptr(tables.count), L.ptr(tables.size), L.ptr(tables.total), V, G, kind, min_count,
                                      m, ptr(ws, ws_off), L.ptr(out), L.ptr(out), L.ptr(out), L.stream_ptr())
        return rc, lib().cc_last_error_string()
    for kw in (dict(V=0), dict(G=0), dict(G=MAX_G + 1), dict(kind=3), dict(kind=-1), dict(min_count=-1), dict(m=0),
               dict(m=1025), dict(ws_off=2)):
        rc, msg = top(**kw)
        assert rc == -1 and b'cc_group_cards_top' in msg, kw
    torch.cuda.synchronize()
    assert bool((ws == 0).all()) and bool((unguarded_t(out) == JUNK_I).all())
    for t in (tables.count, tables.size, tables.total):
        assert bool((unguarded_t(t) == JUNK_I).all())


def unguarded_t(t):
    import torch
    return torch.from_numpy(unguarded(t))
