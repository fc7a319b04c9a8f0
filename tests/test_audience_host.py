"""CPU tests of the card audience's host side: the six bindings against the header, the size
functions (the query workspace never grows with T x N), every argument check of cc_audience_put and
cc_audience_fp32 with never-dereferenced pointers (each call either fails or launches nothing),
CubeCorpus's and api.card_audience's own checks with the library replaced by a stub, the CLI's
arguments, and the CPU reference against oracle/infer_ref.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api, audience
from oracle import infer_ref, model_ref
from tests import audience_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'cc_audience_corpus_size': 3, 'cc_audience_put_ws_size': 3, 'cc_audience_put': 15, 'cc_audience_max_k': 0,
       'cc_audience_ws_size': 5, 'cc_audience_fp32': 17}


def header_args(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return [a.strip() for a in args.split(',') if a.strip() and a.strip() != 'void']


def test_signatures_match_the_header():
    i32, P, SZ, F = C.c_int32, C.c_void_p, C.c_size_t, C.c_float
    assert L.SIGNATURES['cc_audience_corpus_size'] == (SZ, [i32, i32, i32])
    assert L.SIGNATURES['cc_audience_put_ws_size'] == (SZ, [i32, i32, i32])
    assert L.SIGNATURES['cc_audience_put'] == (C.c_int, [P, i32, i32, P, i32, i32, i32, i32, i32, P, P, i32, i32, P, P])
    assert L.SIGNATURES['cc_audience_max_k'] == (i32, [])
    assert L.SIGNATURES['cc_audience_ws_size'] == (SZ, [i32, i32, i32, i32, i32])
    assert L.SIGNATURES['cc_audience_fp32'] == (C.c_int, [P, i32, i32, P, i32, i32, i32, P, i32, i32, i32, F, P, P, P,
                                                          P, P])
    lib = L.lib()
    for name, count in NEW.items():
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):       # a pointer where the header has one
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert lib.cc_abi_version() == 2


def test_workspace_never_grows_with_cards_times_corpus():
    lib = L.lib()
    ws = lambda N, d, T, k, chunk: int(lib.cc_audience_ws_size(N, d, T, k, chunk))   # noqa: E731
    assert int(lib.cc_audience_max_k()) >= 1024
    # an eighth of the 256 MiB a [T][N] key matrix would take
    assert ws(1 << 20, 512, 64, 100, 0) < (64 * (1 << 20) * 4) // 8
    # N doubles at fixed T, k and chunk, from one whole chunk on: the keys stay [T][chunk] and only
    # the candidates grow, by T * k * 8 bytes per added chunk (and one 256-byte rounding)
    for T, k, chunk, first in ((64, 100, 0, 1 << 16), (64, 40, 1024, 1024), (7, 1024, 64, 64), (130, 1, 4096, 4096)):
        step = chunk or first
        N = first
        while N < (1 << 22):
            grown, added_chunks = ws(2 * N, 512, T, k, chunk) - ws(N, 512, T, k, chunk), N // step
            assert 0 < grown <= added_chunks * T * k * 8 + 256, (T, k, chunk, N)
            N *= 2
    # below one chunk the keys are [T][N rounded up to 64]: never more than [T][chunk]
    for chunk in (64, 1024, 0):
        whole = chunk or (1 << 16)
        for N in (1, 63, 64, 65, 300, 1000):
            if N <= whole:
                assert ws(N, 512, 64, 40, chunk) <= ws(whole, 512, 64, 40, chunk), (N, chunk)


def test_size_functions_are_monotone_and_256_byte_multiples():
    """Monotone in every argument the callers grow a kept buffer by (N, d, T, k; the corpus's and
    the put's own).  chunk trades the key term against the candidate term, so it is held to those
    two terms instead."""
    lib = L.lib()
    ws = lambda *a: int(lib.cc_audience_ws_size(*a))               # noqa: E731
    base = dict(N=5000, d=128, T=130, k=40, chunk=1024)
    steps = dict(N=(1, 63, 64, 65, 1024, 1025, 5000, 70000, 1 << 20), d=(64, 128, 512, 1024),
                 T=(1, 7, 64, 65, 130, 512, 4096), k=(1, 2, 40, 100, 1024))
    for name, values in steps.items():
        for chunk in (64, 1024, 0):
            sizes = [ws(*{**base, 'chunk': chunk, name: v}.values()) for v in values]
            assert sizes == sorted(sizes) and all(s % 256 == 0 and s > 0 for s in sizes), (name, chunk)
    for chunk in (64, 128, 1024, 65536, 0):
        N, d, T, k = 5000, 128, 130, 40
        eff, Tp = chunk or 65536, 192
        keys, cand = T * min(eff, -(-N // 64) * 64) * 4, T * k * -(-N // eff) * 8
        fixed = d * Tp * 4 + 3 * Tp * 4                            # the gathered columns, biases, cards, counts
        assert keys + cand + fixed <= ws(N, d, T, k, chunk) <= keys + cand + fixed + 6 * 256
    caps, cards, ds = (1, 63, 64, 65, 700, 65536, 1 << 20), (1, 100, 12345, 1 << 24), (64, 128, 512, 1024)
    size = lambda *a: int(lib.cc_audience_corpus_size(*a))         # noqa: E731
    for d in ds:
        for cc in cards:
            sizes = [size(cap, cc, d) for cap in caps]
            assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
            assert all(s >= cap * d * 4 + (cap + 1) * 4 + cc * 4 for s, cap in zip(sizes, caps))
    for cap in caps:
        assert [size(cap, cc, 128) for cc in cards] == sorted(size(cap, cc, 128) for cc in cards)
        assert [size(cap, 100, d) for d in ds] == sorted(size(cap, 100, d) for d in ds)
    assert size(1 << 16, 1 << 20, 512) <= (1 << 16) * 512 * 4 + ((1 << 16) + 1) * 4 + (1 << 20) * 4 + 3 * 256
    put = lambda *a: int(lib.cc_audience_put_ws_size(*a))          # noqa: E731
    for args, name, values in (((None, 128, 97), 0, (1, 7, 100, 4096)), ((100, None, 97), 1, (64, 128, 1024)),
                               ((100, 128, None), 2, (0, 1, 32, 33, 64, 65, 360, 1000))):
        sizes = [put(*[v if i == name else a for i, a in enumerate(args)]) for v in values]
        assert sizes == sorted(sizes) and all(s % 256 == 0 and s > 0 for s in sizes), name
    assert put(100, 128, 97) >= 100 * 4 * 128 * 4 + 100 * 64 * 4   # ceil(97 / 32) chunk partials and the latents


def failed(entry, what):
    msg = L.lib().cc_last_error_string()
    return entry in msg and what in msg


def test_query_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    cap = int(lib.cc_audience_max_k())

    def ask(params=one, V=1001, d=128, corpus=one, cap_=700, N=300, T=2, cards=one, k=10, chunk=0, members=0,
            threshold=0.5, ws=one, out_idx=one, out_p=one, out_counts=one):
        return lib.cc_audience_fp32(params, V, d, corpus, cap_, N, T, cards, k, chunk, members, threshold, ws, out_idx,
                                    out_p, out_counts, None)
    bad = [(dict(params=None), b'null'), (dict(corpus=None), b'null'), (dict(cards=None), b'null'),
           (dict(ws=None), b'null'), (dict(out_idx=None), b'null'), (dict(out_p=None), b'null'),
           (dict(out_counts=None), b'null'), (dict(k=0), b'k must be'), (dict(k=-2), b'k must be'),
           (dict(k=cap + 1), b'k must be'), (dict(N=0), b'N must be'), (dict(N=-1), b'N must be'),
           (dict(N=701), b'N must be'), (dict(V=0), b'V/cap'), (dict(cap_=0, N=1), b'V/cap'),
           (dict(d=0), b'd must be'), (dict(d=96), b'd must be'), (dict(d=2048), b'd must be'),
           (dict(chunk=-64), b'chunk'), (dict(chunk=1), b'chunk'), (dict(chunk=65), b'chunk'), (dict(chunk=96), b'chunk'),
           (dict(chunk=(1 << 20) + 64), b'chunk'), (dict(threshold=-0.1), b'threshold'), (dict(threshold=1.5), b'threshold'),
           (dict(threshold=float('nan')), b'threshold'),
           (dict(ws=C.c_void_p(4096 + 8)), b'aligned'), (dict(ws=C.c_void_p(4096 + 128)), b'aligned'),
           (dict(corpus=C.c_void_p(4096 + 64)), b'aligned'), (dict(T=-1), b'T outside'), (dict(T=4097), b'T outside')]
    for kw, what in bad:
        assert ask(**kw) == -1 and failed(b'cc_audience_fp32', what), kw
        if 'T' not in kw:                        # a failing call with no cards still fails
            assert ask(**kw, T=0) == -1 and failed(b'cc_audience_fp32', what), kw
    # T == 0: CC_OK, nothing launched
    assert ask(T=0) == 0 and ask(T=0, k=cap, chunk=64, members=1, threshold=1.0) == 0
    assert ask(T=0, N=700, cap_=700) == 0 and ask(T=0, N=1, cap_=1, k=1, threshold=0.0) == 0


def test_put_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)

    def put(params=one, V=1001, d=128, corpus=one, cap_=700, card_cap=5000, n0=0, nnz0=0, R=8, row_ptr=one, idx=one,
            nnz=100, max_n=40, ws=one):
        return lib.cc_audience_put(params, V, d, corpus, cap_, card_cap, n0, nnz0, R, row_ptr, idx, nnz, max_n, ws, None)
    bad = [(dict(params=None), b'null'), (dict(corpus=None), b'null'), (dict(row_ptr=None), b'null'),
           (dict(idx=None), b'null'), (dict(ws=None), b'null'), (dict(corpus=C.c_void_p(4096 + 8)), b'aligned'),
           (dict(ws=C.c_void_p(4096 + 128)), b'aligned'), (dict(V=0), b'V/cap'), (dict(cap_=0), b'V/cap'),
           (dict(card_cap=0), b'V/cap'), (dict(d=0), b'd must be'), (dict(d=100), b'd must be'),
           (dict(d=1088), b'd must be'),
           (dict(n0=-1), b'inside [0, cap)'), (dict(R=-1), b'inside [0, cap)'), (dict(n0=693), b'inside [0, cap)'),
           (dict(n0=700, R=1), b'inside [0, cap)'), (dict(n0=2**31 - 1, R=2**31 - 1), b'inside [0, cap)'),
           (dict(nnz0=-1), b'card_cap'), (dict(nnz=-1), b'card_cap'), (dict(nnz0=4901), b'card_cap'),
           (dict(nnz0=5000, nnz=1), b'card_cap'), (dict(nnz0=2**31 - 1, nnz=2**31 - 1, card_cap=2**31 - 1), b'card_cap'),
           (dict(max_n=-1), b'max_n'), (dict(max_n=1002), b'max_n'), (dict(nnz=321), b'max_n'),
           (dict(R=65536, cap_=70000, nnz=0), b'65535')]
    for kw, what in bad:
        assert put(**kw) == -1 and failed(b'cc_audience_put', what), kw
    # R == 0: CC_OK, nothing launched, anywhere inside the capacities
    assert put(R=0, nnz=0) == 0 and put(R=0, nnz=0, n0=700, nnz0=5000) == 0 and put(R=0, nnz=0, n0=123, max_n=0) == 0
    assert put(R=0, nnz=0, n0=701) == -1 and failed(b'cc_audience_put', b'inside [0, cap)')
    assert put(R=0, nnz=0, nnz0=5001) == -1 and failed(b'cc_audience_put', b'card_cap')


class Stub:
    """Stands in for the _lib module inside audience: the cap may be asked for, every other use of
    the library is recorded and fails."""

    def __init__(self, cap=1024):
        self.calls, self.cap = [], cap

    def lib(self):
        return self

    def cc_audience_max_k(self):
        return self.cap

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            raise AssertionError(f'the library was used: {name}')
        return record


class NoRecommender:
    """What CubeCorpus reads off a Recommender before it launches anything."""
    V, d, dev, stream, params = 50, 64, 'cuda', None, None


def empty_corpus(monkeypatch, N=0, nnz=0, capacity=None, card_capacity=None):
    stub = Stub()
    monkeypatch.setattr(audience, 'L', stub)
    corpus = audience.CubeCorpus(NoRecommender(), capacity=capacity, card_capacity=card_capacity)
    corpus.N, corpus.nnz = N, nnz                # as if N cubes of nnz cards had been put
    return corpus, stub


def test_construction_and_add_check_before_any_library_call(monkeypatch):
    corpus, stub = empty_corpus(monkeypatch)
    assert len(corpus) == 0 and corpus.capacity == 1 and corpus.card_capacity == 1      # at least 1
    sized = empty_corpus(monkeypatch, capacity=7, card_capacity=90)[0]
    assert (sized.capacity, sized.card_capacity) == (7, 90)
    for kw in (dict(capacity=0), dict(capacity=-1), dict(card_capacity=0), dict(card_capacity=-5)):
        with pytest.raises(ValueError, match='capacity'):
            audience.CubeCorpus(NoRecommender(), **kw)
    for bad in ([[1, 2], [3, 50]], [[-1]], [[], [0, 10**6]]):
        with pytest.raises(ValueError, match=r'cube 1|cube 0'):
            audience.CubeCorpus(NoRecommender(), bad)
        with pytest.raises(ValueError, match='outside'):
            corpus.add(bad)
    with pytest.raises(ValueError, match='capacity 2'):        # three cubes into a capacity of two
        audience.CubeCorpus(NoRecommender(), [[1], [2], [3]], capacity=2)
    with pytest.raises(ValueError, match='card_capacity 3'):   # four distinct cards into three slots
        audience.CubeCorpus(NoRecommender(), [[1, 2, 2], [2, 3]], capacity=2, card_capacity=3)
    corpus, stub = empty_corpus(monkeypatch, N=5, nnz=40, capacity=6, card_capacity=42)
    with pytest.raises(ValueError, match='capacity 6'):
        corpus.add([[1], [2]])
    with pytest.raises(ValueError, match='card_capacity 42'):
        corpus.add([[1, 2, 3, 3, 1]])
    assert corpus.add([]) == range(5, 5) and len(corpus) == 5 and corpus.nnz == 40
    model = type('Model', (), {'recommender': lambda self: NoRecommender()})()
    assert audience.CubeCorpus(model, capacity=3).V == 50       # a model or its recommender
    assert stub.calls == []


def test_audience_checks_before_any_library_call(monkeypatch):
    corpus, stub = empty_corpus(monkeypatch, N=10, nnz=100, capacity=16, card_capacity=200)
    for bad in ([3, 50], [-1], [0, 1, 10**6], np.array([49, 50])):
        with pytest.raises(ValueError, match='outside'):
            corpus.audience(bad, 5)
    with pytest.raises(ValueError, match=r'query 1.*50'):
        corpus.audience([3, 50, -1], 5)
    with pytest.raises(ValueError, match=r'1025.*cc_audience_max_k\(\) = 1024'):
        corpus.audience([1], 1025)
    for threshold in (-0.01, 1.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='threshold'):
            corpus.audience([1], 5, threshold=threshold)
    for chunk in (-64, 1, 96, (1 << 20) + 64):
        with pytest.raises(ValueError, match='chunk'):
            corpus.audience([1], 5, chunk=chunk)
    assert stub.calls == []


def test_empty_results_need_no_launch(monkeypatch):
    corpus, stub = empty_corpus(monkeypatch, N=10, nnz=100, capacity=16, card_capacity=200)
    out = corpus.audience([], 7)
    assert sorted(out) == ['above', 'candidates', 'cubes', 'found', 'members', 'probs']
    assert out['cubes'].shape == (0, 7) and out['cubes'].dtype == np.int32
    assert out['probs'].shape == (0, 7) and out['probs'].dtype == np.float32
    assert corpus.audience([], 80)['cubes'].shape == (0, 10)     # n = min(k, N)
    assert corpus.audience([], 0)['cubes'].shape == (0, 0) and corpus.audience([], -3)['probs'].shape == (0, 0)
    for name in ('found', 'members', 'candidates', 'above'):
        assert out[name].shape == (0,) and out[name].dtype == np.int32
    none, stub2 = empty_corpus(monkeypatch)
    out = none.audience([1, 2, 2], 5)                            # an empty corpus: nobody to ask
    assert out['cubes'].shape == (3, 0) and out['probs'].shape == (3, 0)
    for name in ('found', 'members', 'candidates', 'above'):
        assert out[name].tolist() == [0, 0, 0] and out[name].dtype == np.int32
    assert stub.calls == [] and stub2.calls == []


class FakeCorpus:
    def __init__(self):
        self.asked = None

    def audience(self, cards, k, include_members=False):
        self.asked = (list(cards), k, include_members)
        T = len(cards)
        cubes = np.tile(np.array([4, 0, -1], np.int32), (T, 1))
        probs = np.tile(np.array([0.75, 0.5, 0.0], np.float32), (T, 1))
        return {'cubes': cubes, 'probs': probs, 'found': np.array([2] * T, np.int32)}


def test_api_card_audience():
    card_to_int = {'lightning bolt': 3, 'island': 9}
    corpus = FakeCorpus()
    got = api.card_audience(corpus, ['Lightning Bolt', 'island', 'Island'], 3, card_to_int)
    assert corpus.asked == ([3, 9, 9], 3, False)
    assert got == [[(4, 0.75), (0, 0.5)]] * 3                    # the -1 / 0 tail is dropped
    names = {0: 'zero', 4: 'four'}
    got = api.card_audience(corpus, ['island'], 2, card_to_int, cube_names=names, include_members=True)
    assert got == [[('four', 0.75), ('zero', 0.5)]] and corpus.asked == ([9], 2, True)
    corpus.asked = None
    with pytest.raises(KeyError, match='Black Lotus'):
        api.card_audience(corpus, ['island', 'Black Lotus'], 2, card_to_int)
    assert corpus.asked is None                                  # nothing was asked
    assert api.card_audience(corpus, [], 2, card_to_int) == []


def test_cli_arguments(capsys):
    sys.path.insert(0, ROOT)
    from scripts import card_audience as cli
    a = cli.parse_args(['high_req', 'Lightning Bolt', 'Island'])
    assert (a.name, a.cards, a.k, a.include_members, a.threshold, a.synthetic) == \
        ('high_req', ['Lightning Bolt', 'Island'], 20, False, 0.5, None)
    assert (a.data_dir, a.out_dir, a.seed) == ('./data', './ml_files', 0)
    a = cli.parse_args(['m', '3', '9', '3', '--k', '5', '--include-members', '--threshold', '0.25', '--synthetic', '700',
                        '300', '--seed', '4', '--data-dir', 'd', '--out-dir', 'o'])
    assert (a.cards, a.k, a.include_members, a.threshold, a.synthetic, a.seed, a.data_dir, a.out_dir) == \
        ([3, 9, 3], 5, True, 0.25, [700, 300], 4, 'd', 'o')
    for bad in (['m'], [], ['m', 'x', '--k', 'five'], ['m', 'x', '--threshold', '1.5'], ['m', 'x', '--threshold', '-1'],
                ['m', 'Island', '--synthetic', '700', '300'], ['m', 'x', '--synthetic', '700']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()


def test_reference_is_the_forward_pass_at_the_asked_columns():
    V, d = 63, 64
    P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
    rng = np.random.default_rng(5)
    cubes = [rng.choice(V, n, replace=False) for n in (0, 1, 31, 33, 63)]
    cubes.append(np.array([5, 9, 5, 2, 9, 40]))                  # unsorted, with duplicates
    cards = np.array([7, 0, 62, 7, 33], np.int64)
    h3 = R.h3_rows(P, cubes)
    got = R.probs_at(P, h3, cards)
    assert got.dtype == np.float32 and got.shape == (len(cubes), len(cards))
    for r, cube in enumerate(cubes):
        want = infer_ref.recommend_probs(P, cube)[cards]
        assert np.array_equal(R.u32(got[r]), R.u32(want)), r
    ref = R.Ref(P, cubes, V)
    assert np.array_equal(R.u32(ref.p[:, cards]), R.u32(got))
    ci, cp, counts = ref.expected([7, 7, 5, 99, -1], 4)
    assert np.array_equal(ci[0], ci[1]) and np.all(ci[3:] == -1) and np.all(counts[3:] == 0)
    assert counts[2].tolist()[:2] == [int(ref.member[:, 5].sum()), len(cubes) - int(ref.member[:, 5].sum())]
    order = np.lexsort((np.arange(len(cubes)), -ref.p[:, 7]))
    order = order[~ref.member[order, 7]][:4]
    assert ci[0, :len(order)].tolist() == order.tolist()
