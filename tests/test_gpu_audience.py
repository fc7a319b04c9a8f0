"""Card audience on the GPU (cc_audience_put, cc_audience_fp32, CubeCorpus): every index,
probability and count against the CPU reference (tests/audience_ref.py over oracle/infer_ref.py)
and against the device's own forward pass (recommend_many, leave_one_out), bit for bit on uint32
views.  Direct calls run on junk-filled corpus, workspace and outputs with a guard word behind
every output, twice with different junk.

The kernels' own edges, beside the shapes every case runs:
  corpus chunk (64, 128, default)  -> N in {63, 64, 65} (one chunk, exactly, one cube more), 300 and
                                      1029 (a last chunk of 44 / 5 cubes), 2504 (40 chunks of 64)
  score tile 64 cubes x 64 cards   -> the same N; T in {1, 7, 64, 65, 130}, duplicates inside a
                                      tile and across tiles
  gather chunk 32                  -> cubes of 0, 1, 31, 32, 33, 64, 65, 97 cards
  dot chunk 64 / stage 32          -> d = 64, 128, and 1024 (16 chunks, the widest wT)
  k against a chunk's population   -> k = 1, 40, the cap (above every chunk), min(N, cap) (above
                                      the candidates: the -1 / 0 tail)"""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.audience import CubeCorpus
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes
from oracle import model_ref
from tests import audience_ref as R
from tests.audience_ref import u32

pytestmark = pytest.mark.gpu

GUARD = 0x5EEDC0DE
JUNK_I, JUNK_F = -77777, np.float32(-123.25)
JUNKS = (0x7FC0BEEF, 0x0BADF00D)
SIZES = (33, 0, 1, 31, 32, 64, 65, 97)
TWINS = (len(SIZES), len(SIZES) + 1)           # two identical cubes: equal p for every card
_models, _cases = {}, {}


def lib():
    return L.lib()


def max_k():
    return int(lib().cc_audience_max_k())


def model_of(V, d):
    if (V, d) not in _models:
        P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
        _models[(V, d)] = (P, Recommender(Layout(V, d).pack(P), V, d))
    return _models[(V, d)]


def make_cubes(V, N, seed):
    """N cubes: one of each size of SIZES (capped at V), two identical cubes, at V = 63 one cube of
    all 63 cards, then random cubes of up to 50 cards."""
    rng = np.random.default_rng(seed)
    cubes = [rng.choice(V, min(n, V), replace=False) for n in SIZES]
    twin = rng.choice(V, min(V, 21), replace=False)
    cubes += [twin, twin.copy()]
    if V == 63:
        cubes.append(rng.permutation(V))
    while len(cubes) < N:
        cubes.append(rng.choice(V, int(rng.integers(0, min(V, 50) + 1)), replace=False))
    return cubes[:N]


def make_cards(V, T, seed):
    """T query cards with duplicates inside a card tile and across tiles."""
    cards = np.random.default_rng(seed).integers(0, V, T)
    if T > 1:
        cards[1] = cards[0]
    if T > 64:
        cards[T - 1] = cards[0]
        cards[64] = cards[3]
    return cards.astype(np.int32)


def junk_buffer(nbytes, junk):
    buf = torch.full((int(nbytes) // 4 + 64,), junk if junk < 2**31 else junk - 2**32, device='cuda',
                     dtype=torch.int32)
    assert buf.data_ptr() % 256 == 0
    return buf


class Corpus:
    """A junk-filled corpus buffer for a model, and its puts (appended, like CubeCorpus's)."""

    def __init__(self, rec, cap, card_cap, junk=JUNKS[0]):
        self.rec, self.cap, self.card_cap, self.N, self.nnz = rec, cap, card_cap, 0, 0
        self.buf = junk_buffer(lib().cc_audience_corpus_size(cap, card_cap, rec.d), junk)

    def put(self, cubes, junk=JUNKS[1]):
        rec = self.rec
        row_ptr, idx, max_n, _, _ = pack_cubes(cubes, rec.V)
        rp = torch.from_numpy(row_ptr).cuda()
        ix = torch.from_numpy(idx if len(idx) else np.zeros(1, np.int32)).cuda()
        ws = junk_buffer(lib().cc_audience_put_ws_size(len(cubes), rec.d, max_n), junk)
        rc = lib().cc_audience_put(L.ptr(rec.params), rec.V, rec.d, L.ptr(self.buf), self.cap, self.card_cap, self.N,
                                   self.nnz, len(cubes), L.ptr(rp), L.ptr(ix), len(idx), max_n, L.ptr(ws), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, lib().cc_last_error_string()
        self.N, self.nnz = self.N + len(cubes), self.nnz + len(idx)
        return self

    def bits(self):
        return self.buf.cpu().numpy().copy()


def ask(corpus, N, cards, k, chunk=0, members=False, threshold=0.5, junk=JUNKS[0]):
    """A direct cc_audience_fp32 call on junk-filled outputs and workspace with a guard word behind
    every output: (cubes [T, k], probs [T, k], counts [T, 3]); the call succeeded and the guards are
    intact."""
    rec, T = corpus.rec, len(cards)
    c_d = torch.from_numpy(np.asarray(cards, np.int32)).cuda()
    ws = junk_buffer(lib().cc_audience_ws_size(N, rec.d, T, k, chunk), junk)
    oi = torch.full((T * k + 1,), JUNK_I, device='cuda', dtype=torch.int32)
    op = torch.full((T * k + 1,), float(JUNK_F), device='cuda', dtype=torch.float32)
    oc = torch.full((T * 3 + 1,), JUNK_I, device='cuda', dtype=torch.int32)
    oi[-1] = GUARD
    oc[-1] = GUARD
    op[-1] = float(np.array([GUARD], np.uint32).view(np.float32)[0])
    rc = lib().cc_audience_fp32(L.ptr(rec.params), rec.V, rec.d, L.ptr(corpus.buf), corpus.cap, N, T, L.ptr(c_d), k, chunk,
                                1 if members else 0, float(threshold), L.ptr(ws), L.ptr(oi), L.ptr(op), L.ptr(oc),
                                L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().cc_last_error_string()
    oi_h, op_h, oc_h = oi.cpu().numpy(), op.cpu().numpy(), oc.cpu().numpy()
    assert oi_h[-1] == GUARD and op_h[-1:].view(np.uint32)[0] == GUARD and oc_h[-1] == GUARD
    return oi_h[:-1].reshape(T, k), op_h[:-1].reshape(T, k), oc_h[:-1].reshape(T, 3)


def ask_twice(corpus, N, cards, k, **kw):
    """The call with each junk: the two results agree in every bit."""
    a, b = ask(corpus, N, cards, k, junk=JUNKS[0], **kw), ask(corpus, N, cards, k, junk=JUNKS[1], **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(u32(a[1]), u32(b[1])) and np.array_equal(a[2], b[2])
    return a


def assert_rows(got, want, what):
    """Direct rows are [T, k]: the reference's [T, min(k, N)] and the -1 / 0 tail behind it."""
    n = want[0].shape[1]
    assert np.array_equal(got[0][:, :n], want[0]), what
    assert np.array_equal(u32(got[1][:, :n]), u32(want[1])), what
    assert np.all(got[0][:, n:] == -1) and np.all(u32(got[1][:, n:]) == 0), what
    assert np.array_equal(got[2], want[2]), what


class Case:
    """One model, one list of cubes as a corpus on the device, and the reference's probabilities
    of every card for every cube, each once."""

    def __init__(self, V, d, N, seed, cubes=None):
        self.V, self.d, self.N = V, d, N
        self.P, self.rec = model_of(V, d)
        self.cubes = make_cubes(V, N, seed) if cubes is None else cubes
        self.ref = R.Ref(self.P, self.cubes, V)
        nnz = sum(len(np.unique(c)) for c in self.cubes)
        self.corpus = Corpus(self.rec, N + 3, nnz + 5).put(self.cubes)


def case_of(V, d, N, seed):
    if (V, d, N, seed) not in _cases:
        _cases[(V, d, N, seed)] = Case(V, d, N, seed)
    return _cases[(V, d, N, seed)]


def check_prefix(case, N, Ts, seed, chunks=(64, 128, 0)):
    """The first N cubes of the case's corpus: only rows [0, N) are read."""
    cap = max_k()
    for T in Ts:
        cards = make_cards(case.V, T, seed + T)
        for k in sorted({1, 40, cap, min(N, cap)}):
            for members in (False, True):
                want = case.ref.expected(cards, k, include_members=members, N=N)
                for chunk in chunks:
                    got = ask_twice(case.corpus, N, cards, k, chunk=chunk, members=members)
                    assert_rows(got, want, (N, T, k, members, chunk))


@pytest.mark.parametrize('N', [1, 63, 64, 65, 300, 1029])
@pytest.mark.parametrize('V,d', [(63, 64), (1001, 128)])
def test_against_the_oracle(V, d, N):
    check_prefix(case_of(V, d, 1029, seed=V), N, (1, 7, 64, 65, 130), seed=N)


def test_three_chunks_of_k():
    """d = 192, T = 65 cards (a second card tile of one) over N = 65 cubes in two chunks of 64."""
    check_prefix(Case(299, 192, 65, seed=299), 65, (65,), seed=65, chunks=(64,))


def test_forty_chunks():
    check_prefix(case_of(63, 64, 2504, seed=11), 2504, (7, 130), seed=2504, chunks=(64, 0))


def test_wide_model():
    """d = 1024: 16 k-chunks in every dot, and the widest gathered columns."""
    V, d, N = 4100, 1024, 65
    rng = np.random.default_rng(3)
    cubes = [rng.choice(V, n, replace=False) for n in rng.integers(0, 98, N)]
    case = Case(V, d, N, 0, cubes=cubes)
    cards = make_cards(V, 65, 9)
    cards[5] = cubes[2][0]                                                 # a card some cube plays
    for k in (40, N):
        for members in (False, True):
            want = case.ref.expected(cards, k, include_members=members)
            for chunk in (64, 0):
                assert_rows(ask_twice(case.corpus, N, cards, k, chunk=chunk, members=members), want, (k, members, chunk))


def test_identical_cubes_rank_lower_id_first():
    case = case_of(63, 64, 1029, seed=63)
    a, b = TWINS
    assert np.array_equal(np.sort(case.cubes[a]), np.sort(case.cubes[b]))
    outside = np.setdiff1d(np.arange(63), case.cubes[a])[:5].astype(np.int32)
    for N, chunk in ((300, 64), (300, 0), (1000, 128)):
        gi, gp, _ = ask_twice(case.corpus, N, outside, N, chunk=chunk)
        assert_rows((gi, gp, _), case.ref.expected(outside, N, N=N), (N, chunk))
        for t in range(len(outside)):
            pa, pb = int(np.flatnonzero(gi[t] == a)[0]), int(np.flatnonzero(gi[t] == b)[0])
            assert pb == pa + 1 and u32(gp[t, pa:pa + 1])[0] == u32(gp[t, pb:pb + 1])[0]


def test_a_card_in_every_cube_and_a_card_in_none():
    V, d, N = 63, 64, 130
    rng = np.random.default_rng(21)
    cubes = []
    for _ in range(N):
        c = rng.choice(V, int(rng.integers(1, 40)), replace=False)
        cubes.append(np.union1d(c[c != 7], [5]))                           # card 5 always, card 7 never
    case = Case(V, d, N, 0, cubes=cubes)
    cards = np.array([5, 7, 5, 20], np.int32)
    for chunk in (64, 0):
        for k in (1, 40, N):
            gi, gp, gc = ask_twice(case.corpus, N, cards, k, chunk=chunk)
            assert_rows((gi, gp, gc), case.ref.expected(cards, k), (k, chunk))
            assert gc[0].tolist() == [N, 0, 0] and np.all(gi[0] == -1) and np.all(u32(gp[0]) == 0)
            assert gc[1].tolist()[:2] == [0, N] and np.all(gi[1] >= 0)
            got = ask_twice(case.corpus, N, cards, k, chunk=chunk, members=True)
            assert_rows(got, case.ref.expected(cards, k, include_members=True), (k, chunk, 'members'))
            assert got[2][0].tolist()[:2] == [N, N] and np.all(got[0][0] >= 0)


def test_an_out_of_range_card_gives_an_empty_row():
    case = case_of(63, 64, 1029, seed=63)
    N, k = 300, 12
    cards = np.array([3, 63, 9, -1, 2**31 - 1, 3, -2**31], np.int64).astype(np.int32)
    valid = (cards >= 0) & (cards < 63)
    want = case.ref.expected(cards, k, N=N)
    for chunk in (64, 0):
        gi, gp, gc = ask_twice(case.corpus, N, cards, k, chunk=chunk)
        assert_rows((gi, gp, gc), want, chunk)
        assert np.all(gi[~valid] == -1) and np.all(u32(gp[~valid]) == 0) and np.all(gc[~valid] == 0)
        assert np.all(gi[valid][:, 0] >= 0)


def test_threshold_counts():
    case = case_of(1001, 128, 1029, seed=1001)
    N, k = 300, 5
    cards = make_cards(1001, 7, 77)
    first = case.ref.expected(cards, k, N=N)
    exact = float(first[1][2, 3])                          # the probability of one candidate cube
    above = np.nextafter(np.float32(exact), np.float32(2))
    for members in (False, True):
        for chunk in (64, 0):
            for threshold in (0.0, 1.0, exact, float(above), 0.5):
                want = case.ref.expected(cards, k, include_members=members, threshold=threshold, N=N)
                got = ask_twice(case.corpus, N, cards, k, chunk=chunk, members=members, threshold=threshold)
                assert_rows(got, want, (members, chunk, threshold))
                if threshold == 0.0:
                    assert np.array_equal(got[2][:, 2], got[2][:, 1])
            at = ask(case.corpus, N, cards, k, chunk=chunk, members=members, threshold=exact)[2][2, 2]
            over = ask(case.corpus, N, cards, k, chunk=chunk, members=members, threshold=float(above))[2][2, 2]
            assert at > over                               # >= counts the cube at the threshold itself


def test_piecewise_puts():
    """Puts of 100-row pieces against one put: the same corpus buffer and the same answers."""
    case = case_of(63, 64, 1029, seed=63)
    N = 300
    cubes = case.cubes[:N]
    nnz = sum(len(np.unique(c)) for c in cubes)
    whole = Corpus(case.rec, N, nnz, JUNKS[0]).put(cubes, junk=JUNKS[0])
    pieces = Corpus(case.rec, N, nnz, JUNKS[0])
    for n0 in (0, 100, 200):
        pieces.put(cubes[n0:n0 + 100], junk=JUNKS[1])
    pieces.put([])                                          # no rows: nothing
    odd = Corpus(case.rec, N, nnz, JUNKS[0])
    for n0, n1 in ((0, 1), (1, 129), (129, 130), (130, 300)):
        odd.put(cubes[n0:n1])
    assert np.array_equal(whole.bits(), pieces.bits()) and np.array_equal(whole.bits(), odd.bits())
    cards = make_cards(63, 65, 5)
    want = case.ref.expected(cards, 40, N=N)
    for corpus in (whole, pieces, odd):
        for chunk in (64, 0):
            assert_rows(ask_twice(corpus, N, cards, 40, chunk=chunk), want, chunk)


def test_agrees_with_the_forward_pass_on_the_device():
    """CubeCorpus.audience's probabilities are recommend_many's probs at those cards and
    leave_one_out's base."""
    V, d, N = 1001, 128, 65
    case = case_of(V, d, 1029, seed=V)
    cubes = case.cubes[:N]
    corpus = CubeCorpus(case.rec, cubes)
    cards = make_cards(V, 7, 3)
    out = corpus.audience(cards, N, include_members=True)
    assert np.all(out['found'] == N) and np.all(out['candidates'] == N)
    many = case.rec.recommend_many(cubes, 1, want_probs=True)
    loo = case.rec.leave_one_out(cubes, targets=cards)
    for t, card in enumerate(cards.tolist()):
        for j, p in zip(out['cubes'][t].tolist(), out['probs'][t]):
            assert u32(p)[0] == u32(many[j]['probs'][card])[0] == u32(loo[j]['base'][t])[0], (t, j)
    want = case.ref.expected(cards, N, include_members=True, N=N)
    assert np.array_equal(out['cubes'], want[0]) and np.array_equal(u32(out['probs']), u32(want[1]))


def same_results(a, b):
    return all(a[key].dtype == b[key].dtype and a[key].shape == b[key].shape
               and np.array_equal(a[key].view(np.uint32) if a[key].dtype == np.float32 else a[key],
                                  b[key].view(np.uint32) if b[key].dtype == np.float32 else b[key]) for key in a)


def test_cube_corpus_does_not_depend_on_the_launches():
    V, d = 63, 64
    case = case_of(V, d, 1029, seed=V)
    rng = np.random.default_rng(8)
    base = rng.choice(V, 30, replace=False)
    messy = rng.permutation(np.concatenate([base, base[:9], base[3:5]]))   # unsorted, with duplicates
    cubes = case.cubes[:299] + [messy]
    ref = R.Ref(case.P, cubes, V)
    corpus = CubeCorpus(case.rec, cubes[:200], capacity=400, card_capacity=20000, rows_per_launch=70)
    assert corpus.add(cubes[200:]) == range(200, 300) and len(corpus) == 300
    cards = make_cards(V, 130, 4)
    whole = corpus.audience(cards, 40, rows_per_launch=4096)
    want = ref.expected(cards, 40)
    assert np.array_equal(whole['cubes'], want[0]) and np.array_equal(u32(whole['probs']), u32(want[1]))
    assert np.array_equal(np.stack([whole['members'], whole['candidates'], whole['above']], 1), want[2])
    assert np.array_equal(whole['found'], np.minimum(want[2][:, 1], 40))
    for rpl in (1, 64, 65):
        assert same_results(corpus.audience(cards, 40, rows_per_launch=rpl), whole), rpl
    assert same_results(corpus.audience(cards, 40, chunk=64), whole)
    assert same_results(corpus.audience(cards, 40, chunk=128, rows_per_launch=7), whole)
    k0 = corpus.audience(cards, 0)                         # no columns, the counts all the same
    assert k0['cubes'].shape == (130, 0) and np.all(k0['found'] == 0)
    assert np.array_equal(k0['candidates'], whole['candidates']) and np.array_equal(k0['members'], whole['members'])
    # more cubes after a query: the next query sees them
    more = [np.array(case.cubes[TWINS[0]]), np.arange(3)]
    assert corpus.add(more) == range(300, 302)
    grown = R.Ref(case.P, cubes + more, V)
    got = corpus.audience(cards, 302, include_members=True, threshold=0.25)
    want = grown.expected(cards, 302, include_members=True, threshold=0.25)
    assert np.array_equal(got['cubes'], want[0]) and np.array_equal(u32(got['probs']), u32(want[1]))
    assert np.array_equal(got['above'], want[2][:, 2]) and np.all(got['found'] == 302)
    with pytest.raises(ValueError, match='capacity 400'):
        corpus.add([[1]] * 99)
    assert len(corpus) == 302
