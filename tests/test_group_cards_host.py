"""CPU tests of the archetype card profiles' host side: the bindings against the header, every
argument check of the three entry points with never-dereferenced pointers, the workspace bound, the
reference (tests/group_cards_ref.py) against exact rational arithmetic, the composite packing at its
limits, GroupCards on the host, the Python checks with the library replaced by a stub, and the
CLI's arguments."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import cubecluster, groupcards
from tests import group_cards_ref as R
from tests.test_cube_index_host import header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'cc_group_cards_tile': 0, 'cc_group_cards_max_groups': 0, 'cc_group_cards_ws_size': 4,
       'cc_group_cards_count': 13, 'cc_group_cards_top': 13, 'cc_audience_corpus_ptr_offset': 2,
       'cc_audience_corpus_ids_offset': 2}


def test_signatures_match_the_header():
    i32, P, SZ = C.c_int32, C.c_void_p, C.c_size_t
    assert L.SIGNATURES['cc_group_cards_ws_size'] == (SZ, [i32, i32, i32, i32])
    assert L.SIGNATURES['cc_group_cards_count'] == (C.c_int, [P, P, i32, i32, P, i32, i32, i32, P, P, P, P, P])
    assert L.SIGNATURES['cc_group_cards_top'] == (C.c_int, [P, P, P, i32, i32, i32, i32, i32, P, P, P, P, P])
    lib = L.lib()
    for name, count in NEW.items():
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):       # a pointer where the header has one
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert int(lib.cc_group_cards_max_groups()) >= 1024
    tile = int(lib.cc_group_cards_tile())
    assert tile >= 22000 and tile * 4 <= 160 * 1024              # a 22,000-card histogram in one CU's LDS
    assert groupcards.KINDS == {k: i for i, k in enumerate(R.KINDS)}
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    assert 'CC_GROUP_RATE = 0, CC_GROUP_LIFT = 1, CC_GROUP_AVOID = 2' in hdr


def test_corpus_offsets_are_the_layout():
    """ptr behind the h3 rows, ids behind ptr, and the corpus size behind ids by the cards."""
    lib = L.lib()
    for cap, d in ((1, 64), (700, 64), (70000, 128), (5, 1024)):
        p, i = int(lib.cc_audience_corpus_ptr_offset(cap, d)), int(lib.cc_audience_corpus_ids_offset(cap, d))
        assert p % 256 == 0 and i % 256 == 0
        assert p >= cap * d * 4 and p - cap * d * 4 < 256 and i >= p + (cap + 1) * 4 and i - p - (cap + 1) * 4 < 256
        for cards in (1, 1000):
            assert int(lib.cc_audience_corpus_size(cap, cards, d)) == i + -(-cards * 4 // 256) * 256


def test_workspace_bound():
    """At or below 4 R + R / 32 + 20 G + 2 KiB bytes: the grouped cube ids and the
    slice list; it depends on neither V nor m, so no [G][V] table of any kind is in it."""
    ws = lambda R_, V, G, m: int(L.lib().cc_group_cards_ws_size(R_, V, G, m))   # noqa: E731
    for R_, V, G, m in ((65536, 22000, 256, 100), (1 << 20, 22000, 1024, 100), (1 << 22, 1 << 18, 1024, 1024),
                        (0, 1, 1, 1), (257, 65, 2, 7), (4096, 22000, 1024, 10)):
        got = ws(R_, V, G, m)
        assert 0 < got <= 4 * R_ + R_ // 32 + 20 * G + 2048 and got % 256 == 0, (R_, V, G, m)
        assert got >= 4 * R_ + 12 * G
        assert got < G * V * 4 or G * V * 4 < (1 << 20), (R_, V, G, m)
    for name, values in dict(R=(0, 1, 255, 256, 257, 70000, 1 << 22), V=(1, 65, 22528, 22529, 1 << 18),
                             G=(1, 2, 65, 1024), m=(1, 7, 1024)).items():
        base = dict(R=5000, V=2000, G=65, m=7)
        sizes = [ws(*{**base, name: v}.values()) for v in values]
        assert sizes == sorted(sizes), name


# ------------------------------------------------------------------ argument checks
def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    cap = int(lib.cc_group_cards_max_groups())

    def failed(entry, what):
        msg = lib.cc_last_error_string()
        return entry in msg and what in msg

    def count(row_ptr=one, idx=one, R_=300, V=500, label=one, G=5, accumulate=0, path=0, ws=one, cnt=one, size=one,
              total=one):
        return lib.cc_group_cards_count(row_ptr, idx, R_, V, label, G, accumulate, path, ws, cnt, size, total, None)
    bad = [(dict(row_ptr=None), b'null'), (dict(idx=None), b'null'), (dict(label=None), b'null'), (dict(ws=None), b'null'),
           (dict(cnt=None), b'null'), (dict(size=None), b'null'), (dict(total=None), b'null'),
           (dict(R_=-1), b'R must be'), (dict(R_=(1 << 22) + 1), b'R must be'), (dict(V=0), b'V must be'),
           (dict(V=-4), b'V must be'), (dict(V=(1 << 18) + 1), b'V must be'), (dict(G=0), b'G must be'),
           (dict(G=-1), b'G must be'), (dict(G=cap + 1), b'G must be'), (dict(accumulate=2), b'accumulate'),
           (dict(accumulate=-1), b'accumulate'), (dict(path=3), b'path'), (dict(path=-1), b'path'),
           (dict(ws=C.c_void_p(4096 + 8)), b'aligned')]
    for kw, what in bad:
        assert count(**kw) == -1 and failed(b'cc_group_cards_count', what), kw
        if 'R_' not in kw:                       # a failing call with no rows still fails
            assert count(**kw, R_=0) == -1 and failed(b'cc_group_cards_count', what), kw
    for path in (0, 1, 2):                       # nothing to add: nothing launched
        assert count(R_=0, accumulate=1, path=path, G=cap, V=1 << 18) == 0

    def top(cnt=one, size=one, total=one, V=500, G=5, kind=1, min_count=1, m=10, ws=one, cards=one, ccnt=one, found=one):
        return lib.cc_group_cards_top(cnt, size, total, V, G, kind, min_count, m, ws, cards, ccnt, found, None)
    bad = [(dict(cnt=None), b'null'), (dict(size=None), b'null'), (dict(total=None), b'null'), (dict(ws=None), b'null'),
           (dict(cards=None), b'null'), (dict(ccnt=None), b'null'), (dict(found=None), b'null'), (dict(V=0), b'V must be'),
           (dict(V=(1 << 18) + 1), b'V must be'), (dict(G=0), b'G must be'), (dict(G=cap + 1), b'G must be'),
           (dict(kind=3), b'kind'), (dict(kind=-1), b'kind'), (dict(min_count=-1), b'min_count'), (dict(m=0), b'm must be'),
           (dict(m=-2), b'm must be'), (dict(m=1025), b'm must be'), (dict(ws=C.c_void_p(4096 + 128)), b'aligned')]
    for kw, what in bad:
        assert top(**kw) == -1 and failed(b'cc_group_cards_top', what), kw
    assert int(lib.cc_group_cards_ws_size(-5, 0, 0, 0)) > 0     # the size of a refused call is still a size


# ------------------------------------------------------------------ the reference against exact rationals
def small_case(seed, R_=40, V=17, G=4):
    rng = np.random.default_rng(seed)
    cubes = [np.sort(rng.choice(V, int(rng.integers(0, V + 1)), replace=False)).astype(np.int32) for _ in range(R_)]
    label = rng.integers(-1, G, R_).astype(np.int32)
    if seed % 2:
        label[label == 2] = -1                   # an empty group
    return cubes, label, V, G


@pytest.mark.parametrize('seed', range(6))
def test_reference_against_rational_arithmetic(seed):
    cubes, label, V, G = small_case(seed)
    row_ptr, idx = R.csr(cubes)
    count, size, total = R.counts(row_ptr, idx, label, V, G)
    want = np.zeros((G, V), np.int64)            # the definition, cube by cube
    for c, l in zip(cubes, label.tolist()):
        if l >= 0:
            want[l, c] += 1
    assert np.array_equal(count, want) and np.array_equal(size, np.bincount(label[label >= 0], minlength=G))
    assert np.array_equal(total, want.sum(0)) and count.dtype == np.uint32 and total.dtype == np.uint32
    N = int(size.sum())
    for min_count in (1, 2):
        for m in (3, V + 5):
            for kind in R.KINDS:
                cards, ccnt, found = R.top(count, size, total, kind, min_count, m)
                for g in range(G):
                    s = int(size[g])
                    if s == 0:
                        assert found[g] == 0 and np.all(cards[g] == -1)
                        continue
                    a, t = [int(x) for x in count[g]], [int(x) for x in total]
                    cand = [v for v in range(V) if (t[v] if kind == 'avoid' else a[v]) >= min_count]
                    score = {'rate': lambda v: Fraction(a[v], s), 'lift': lambda v: Fraction(a[v], s) - Fraction(t[v], N),
                             'avoid': lambda v: Fraction(t[v], N) - Fraction(a[v], s)}[kind]
                    order = sorted(cand, key=lambda v: (-score(v), v))[:m]
                    assert found[g] == len(order) and cards[g, :found[g]].tolist() == order
                    assert np.all(cards[g, found[g]:] == -1) and np.all(ccnt[g, found[g]:] == 0)
                    assert ccnt[g, :found[g]].tolist() == [a[v] for v in order]
                    if kind == 'lift' and s < N:  # equally: the in-group rate minus the out-of-group rate
                        out = lambda v: Fraction(a[v], s) - Fraction(t[v] - a[v], N - s)      # noqa: E731
                        assert sorted(cand, key=lambda v: (-out(v), v))[:m] == order
                        k = R.keys(count, size, total, 'lift')
                        assert all(out(v) == Fraction(int(k[g, v]), s * (N - s)) for v in cand)


def test_composite_packing_at_the_limits():
    """N = 2^22, V = 2^18, both signs of the key: the composite fits 64 bits, is unique, stays below
    the select's `no candidate` value, and ascending composites are (key descending, card ascending)."""
    N, V = 1 << 22, 1 << 18
    ks = [N * N, N * N - 1, 1, 0, -1, -(N * N) + 1, -(N * N)]
    assert max(abs(k) for k in ks) == 1 << 44
    items = [(k, c) for k in ks for c in (0, 1, V - 2, V - 1)]
    comps = [R.composite(k, c) for k, c in items]
    assert all(0 < x < (1 << 64) - 1 for x in comps) and len(set(comps)) == len(comps)
    assert [items[i] for i in np.argsort(np.array(comps, np.uint64), kind='stable')] == \
        sorted(items, key=lambda kc: (-kc[0], kc[1]))
    assert all(x & (V - 1) == c and (x >> 18) == (1 << 45) - k for x, (k, c) in zip(comps, items))
    # the keys of real counts stay within a quarter of the limit: a (N - s) <= s (N - s) <= N^2 / 4
    assert max(a * N - t * s for s in (1, N // 2, N - 1) for a in (0, s) for t in (a, a + N - s)) <= N * N // 4


# ------------------------------------------------------------------ the Python surface
def result(kind='lift'):
    cubes, label, V, G = small_case(2)
    count, size, total = R.counts(*R.csr(cubes), label, V, G)
    cards, ccnt, found = R.top(count, size, total, kind, 1, 6)
    return groupcards.GroupCards(cards, ccnt, found, size, total, kind, 1, counts=count), cubes, count, size, total


def test_group_cards_result_on_the_host():
    res, cubes, count, size, total = result()
    N = int(size.sum())
    assert (res.G, res.m, res.V, res.N, res.kind, res.min_count) == (4, 6, 17, N, 'lift', 1)
    for g in range(res.G):
        for i in range(int(res.found[g])):
            v = int(res.cards[g, i])
            assert res.rate[g, i] == count[g, v] / size[g] and res.base[g, i] == total[v] / N
            assert res.lift[g, i] == res.rate[g, i] - res.base[g, i]
        assert np.all(res.rate[g, res.found[g]:] == 0) and np.all(res.lift[g, res.found[g]:] == 0)
    assert res.rate.dtype == res.base.dtype == res.lift.dtype == np.float64
    row = res.list_of(1).tolist()
    assert res.missing(1, [], 99).tolist() == row and res.missing(1, row, 5).tolist() == []
    assert res.missing(1, row[::2], 99).tolist() == row[1::2] and res.missing(1, row[:1], 2).tolist() == row[1:3]
    assert res.missing(1, [999], 0).tolist() == [] and res.missing(1, [], -3).tolist() == []
    for bad in (-1, 4):
        with pytest.raises(ValueError, match='group'):
            res.missing(bad, [], 1)


class Stub:
    """Stands in for the _lib module: the cap may be asked for, every other use fails."""

    def __init__(self):
        self.calls = []

    def lib(self):
        return self

    def cc_group_cards_max_groups(self):
        return 1024

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            raise AssertionError(f'the library was used: {name}')
        return record


def test_python_checks_before_any_library_call(monkeypatch):
    stub = Stub()
    monkeypatch.setattr(groupcards, 'L', stub)
    cubes = [[0, 1], [2], [1, 3], []]
    ok = dict(cubes=cubes, labels=[0, 1, -1, 1], V=5, m=3)
    for kw, what in ((dict(labels=[0, 1, 2]), '3 labels for 4 cubes'), (dict(labels=[0, 1, -2, 1]), r'cube 2: label -2'),
                     (dict(labels=[0, 1, 2, 1], G=2), r'cube 2: label 2 outside \[-1, 2\)'), (dict(m=0), 'm = 0'),
                     (dict(m=1025), 'm = 1025'), (dict(kind='best'), 'kind'), (dict(V=0), 'V = 0'),
                     (dict(V=(1 << 18) + 1), 'V ='), (dict(min_count=-1), 'min_count'), (dict(G=0), 'G = 0'),
                     (dict(G=1025), 'G = 1025'), (dict(labels=[0, 1, 1024, 1]), 'G = 1025'),
                     (dict(cubes=[[0, 1], [2], [1, 5], []]), r'outside \[0, 5\)')):
        with pytest.raises(ValueError, match=what):
            groupcards.group_cards(**{**ok, **kw})
    many = np.zeros((1 << 22) + 1, np.int32)
    with pytest.raises(ValueError, match='labelled cubes'):
        groupcards.check_args(len(many), many, 5, 3, 'lift', 1, None)
    lab, V, m, kind, min_count, G = groupcards.check_args(4, [0, 3, -1, 1], 5, 3, 'rate', 2, None)
    assert lab.dtype == np.int32 and (V, m, kind, min_count, G) == (5, 3, 'rate', 2, 4)
    assert groupcards.check_args(0, [], 5, 3, 'rate', 2, None)[5] == 1
    assert groupcards.check_args(2, [-1, -1], 5, 3, 'avoid', 0, None)[5] == 1

    class Corpus:                                # what corpus_group_cards reads before it launches
        V, dev, N, capacity, d = 5, 'cuda', 4, 4, 64

        def __len__(self):
            return self.N
    for kw, what in ((dict(labels=[0, 1]), '2 labels for 4 cubes'), (dict(labels=[0, 1, 7, 1], G=3), 'label 7'),
                     (dict(labels=[0] * 4, m=0), 'm = 0'), (dict(labels=[0] * 4, kind='x'), 'kind')):
        with pytest.raises(ValueError, match=what):
            groupcards.corpus_group_cards(Corpus(), **{**dict(m=3), **kw})
    # CubeClusters.signature_cards: exactly the clustering's cubes
    labels = np.array([0, 1, 1, 0], np.int32)
    res = cubecluster.CubeClusters(None, np.arange(2), labels, np.zeros(4, np.float32), None,
                                   np.zeros((2, 64), np.float32), np.array([2, 2], np.int32), np.array([4, 0], np.int32), 1)
    for bad in (cubes[:3], cubes + [[1]], type('Five', (Corpus,), {'N': 5})()):
        with pytest.raises(ValueError, match='cubes for a clustering of 4'):
            res.signature_cards(bad, 3)
    assert stub.calls == []


def test_cli_arguments(capsys):
    sys.path.insert(0, ROOT)
    from scripts import archetype_cards as cli
    a = cli.parse_args(['high_req', '40'])
    assert (a.name, a.k, a.m, a.kind, a.min_count, a.seed, a.max_iter, a.n_init, a.synthetic) == \
        ('high_req', 40, 10, 'lift', 1, 0, 50, 1, None)
    assert (a.data_dir, a.out_dir) == ('./data', './ml_files')
    a = cli.parse_args(['m', '5', '--m', '25', '--kind', 'avoid', '--min-count', '4', '--seed', '4', '--max-iter', '9',
                        '--n-init', '3', '--synthetic', '700', '300', '--data-dir', 'd', '--out-dir', 'o'])
    assert (a.k, a.m, a.kind, a.min_count, a.seed, a.max_iter, a.n_init, a.synthetic, a.data_dir, a.out_dir) == \
        (5, 25, 'avoid', 4, 4, 9, 3, [700, 300], 'd', 'o')
    assert cli.parse_args(['m', '5', '--kind', 'rate']).kind == 'rate'
    for bad in (['m'], ['m', 'five'], ['m', '5', '--kind', 'best'], ['m', '5', '--m', 'x'], ['m', '5', '--synthetic', '7']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()
