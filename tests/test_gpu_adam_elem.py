"""The TF Adam update (csrc/adam.hpp, cc_adam::elem) and every launch path that runs it, per element
(run on an MI355X).

cc_adam_dense is the anchor: every regime of tests/adam_ref.py (fresh, trained, absent, eps_band, wide,
ties, each with four alpha probes), at state[0] in {0, 1, 4, 99, 999, 6930, 10^5, 2^24 - 1, 2^31} with
the default hyperparameters and at three of them with (3e-4, 0.8, 0.99, 1e-8), n in {1, 3, 4, 5, 1023,
1024, 1027, 10007}, with and without a shadow:
  (a) m', v', p' inside their derived fp64 bounds at every element (adam_ref docstring: the derivation)
  (b) m', v' equal adam_ref.emulate (numpy float32, operation for operation) bit for bit
  (c) the device's alpha, read off the probes (p = 0, m = g = v = 1: p' = -fl(alpha / fl(1 + eps)), at
      most three fp32 candidates): all probes agree, a candidate lies inside the alpha bound (K = 16 ulp
      of powf amplified by the cancellation in 1 - b^t), and with one candidate p' equals emulate bit
      for bit at every element.  Below n = 16 a range has no room for probes beside the regime's own
      elements: there a second call on n probe elements, same state, reads alpha
  (d) the shadow equals bf16_rne(p') bit for bit (the ties regime: p' = p exactly halfway)
  (e) state, g and 64 sentinel elements on either side of every buffer unchanged
The fused writers (cc_adam_dense_t, cc_tower_bwd_chain_adam, cc_embed_grad_cs_adam,
cc_embed_grad_cs_adam_reg) run on
trained / absent / eps_band / ties at state[0] in {0, 4, 6930} and must equal cc_adam_dense over the
same ranges bit for bit on p, m, v and the shadow, whole buffers (sentinels and everything outside the
ranges included); cc_adam_dense_t's transposed copies are the numpy layout (adam_ref) of that shadow.
So cc_adam_dense is pinned to fp64 directly and the others through bit-equality with it.  The four
Adam + F entries (cc_adam_noise, cc_adam_noise_pack, cc_adam_noise_pack2, cc_adam_pack2) are not
called here: they stay pinned through the trainer tests of test_gpu_train.py alone.  Observed error / bound per step:
DESIGN.md §2.
"""
import ctypes

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from tests import adam_ref as AR
from tests import test_gpu_embed_cs_forms as CS
from tests import tower_ref as TR
from tests.gpu_helpers import record_errors
from tests.test_gpu_tower_elem import _CHAIN, Run

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 7.0
FILL16 = 0x40E0       # 7.0 in bf16
NS = (1, 3, 4, 5, 1023, 1024, 1027, 10007)
# every extern "C" entry whose kernel inlines cc_adam::elem and that this file pins
ENTRIES = {'cc_adam_dense', 'cc_adam_dense_t', 'cc_tower_bwd_chain_adam', 'cc_embed_grad_cs_adam',
           'cc_embed_grad_cs_adam_reg'}
CALLED = set()


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    L.lib()


def _call(name, *args):
    CALLED.add(name)
    L.call(name, *args)


def _state(step, batch=1):
    return torch.tensor([step, batch, 0, 0], device='cuda', dtype=torch.int64)


def _guarded(a, fill):
    """A host array between GUARD sentinel elements on either side, on the device (a plain copy: no
    arithmetic touches a denormal)."""
    g = np.full(GUARD, fill, a.dtype)
    return torch.from_numpy(np.concatenate([g, a, g])).cuda()


class Bufs:
    """p, m, v, g (fp32) and the shadow (bf16 bits as int16, prefilled with FILL16), each between guards."""

    def __init__(self, p, m, v, g):
        self.n = len(p)
        self.t = {k: _guarded(np.asarray(a, np.float32), np.float32(FILL)) for k, a in zip('pmvg', (p, m, v, g))}
        self.t['s'] = _guarded(np.full(self.n, FILL16, np.int16), np.int16(FILL16))
        self._host = {}

    @classmethod
    def of(cls, inp):
        return cls(inp.p, inp.m, inp.v, inp.g)

    def ptr(self, k, lo=0):
        t = self.t[k]
        return ctypes.c_void_p(t.data_ptr() + (GUARD + lo) * t.element_size())

    def pmvgs(self, lo=0, shadow=True):
        return [self.ptr(k, lo) for k in 'pmvg'] + [self.ptr('s', lo) if shadow else None]

    def same(self, other):
        """Names of the buffers that differ anywhere (guards included), bitwise."""
        view = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
        return [k for k in 'pmvgs' if not torch.equal(view(self.t[k]), view(other.t[k]))]

    def host(self, k):
        """The whole buffer on the host (read once, after the last launch)."""
        if k not in self._host:
            a = self.t[k].cpu().numpy()
            self._host[k] = a.view(np.uint16) if k == 's' else a
        return self._host[k]

    def inner(self, k):
        return self.host(k)[GUARD:GUARD + self.n]

    def guards_ok(self):
        for k in 'pmvgs':
            a, f = self.host(k), (FILL16 if k == 's' else np.float32(FILL))
            assert np.all(a[:GUARD] == f) and np.all(a[GUARD + self.n:] == f), f'{k}: sentinel overwritten'


def _dense(b, ranges, step, hp=AR.HP_DEFAULT, shadow=True):
    """cc_adam_dense over each (lo, n) of b."""
    st = _state(step)
    for lo, n in ranges:
        _call('cc_adam_dense', *b.pmvgs(lo, shadow), n, L.ptr(st), *hp, L.stream_ptr())
    torch.cuda.synchronize()
    assert st.tolist() == [step, 1, 0, 0]
    return b


# ---------------------------------------------------------------------------------- cc_adam_dense, the anchor
def _device_alpha(out, inp, step, hp):
    """The candidates for the device's alpha from the probes of `out` (or of a call on probes alone)."""
    if len(inp.probes) == 0:
        pi = AR.probe_inputs(inp.n)
        out = _dense(Bufs.of(pi), [(0, inp.n)], step, hp)
        inp = pi
    pp, mm, vv = (out.inner(k)[inp.probes] for k in 'pmv')
    assert np.all(mm == 1) and np.all(vv == 1), 'a probe\'s m\' or v\' is not exactly 1'
    assert len(set(pp.view(np.uint32).tolist())) == 1, 'the probes disagree on alpha'
    return AR.alpha_candidates(pp[0], hp)


def _check_dense(inp, ref, step, hp, shadow, errs):
    regime, n = inp.regime, inp.n
    out = _dense(Bufs.of(inp), [(0, n)], step, hp, shadow)
    p1, m1, v1 = (out.inner(k) for k in 'pmv')
    tag = (regime, n, step, shadow)
    # (a) the derived fp64 bounds
    r = AR.ratios(ref, p1, m1, v1)
    for k, x in r.items():
        errs[k] = max(errs.get(k, 0.0), x)
    # (c) alpha off the probes
    cands = _device_alpha(out, inp, step, hp)
    ra = [abs(float(a) - ref.alpha) / ref.alpha / ref.ra for a in cands]
    errs['alpha'] = max(errs.get('alpha', 0.0), min(ra))
    assert AR.passes(r), (tag, r)
    assert cands and min(ra) <= 1, (tag, cands, ref.alpha, ref.ra)
    # (b), (c) bit for bit
    em = [AR.emulate(inp.p, inp.m, inp.v, inp.g, a, hp) for a in cands]
    assert AR.same_bits(m1, em[0][1]), (tag, 'm\' differs from the fp32 emulation')
    assert AR.same_bits(v1, em[0][2]), (tag, 'v\' differs from the fp32 emulation')
    assert any(AR.same_bits(p1, e[0]) for e in em), (tag, 'p\' differs from the fp32 emulation for every candidate alpha')
    if step == 2 ** 31:      # b^t = 0: alpha is lr itself (a step cut to 32 bits gives another t)
        assert AR.same_bits(p1, AR.emulate(inp.p, inp.m, inp.v, inp.g, np.float32(hp[0]), hp)[0]), (tag, 'alpha != lr')
    # (d) shadow, (e) untouched
    out.guards_ok()
    assert AR.same_bits(out.inner('g'), inp.g)
    if shadow:
        assert np.array_equal(out.inner('s'), AR.bf16_rne(p1)), (tag, 'shadow')
    else:
        assert np.all(out.inner('s') == FILL16), (tag, 'shadow = NULL but the shadow was written')
    if regime == 'ties':
        free = np.setdiff1d(np.arange(n), inp.probes)
        assert AR.same_bits(p1[free], inp.p[free])
    return r


DENSE = [pytest.param(s, AR.HP_DEFAULT, id=f'step{s}-default') for s in AR.STEPS] + \
        [pytest.param(s, AR.HP_SECOND, id=f'step{s}-second') for s in (0, 999, 2 ** 31)]


@pytest.mark.parametrize('step,hp', DENSE)
def test_adam_dense_elementwise(request, step, hp):
    errs = {}
    for regime in AR.REGIMES:
        for n in NS:
            inp = AR.inputs(regime, n)
            ref = AR.reference(inp.p, inp.m, inp.v, inp.g, step, hp)
            for shadow in (True, False):
                _check_dense(inp, ref, step, hp, shadow, errs)
    print(request.node.name, errs)
    record_errors(request.node.name, step, errs)


@pytest.mark.parametrize('regime', [r for r in AR.REGIMES if r != 'fresh'])
def test_adam_dense_old_anchor_claim(regime):
    """test_adam_matches_tf_formula's claim (|p' - reference| < 1e-6 at t = 5, oracle/model_ref.adam_tf
    in float32) at the other regimes."""
    from oracle import model_ref
    inp = AR.inputs(regime, 10007)
    out = _dense(Bufs.of(inp), [(0, inp.n)], 4, shadow=False)
    with np.errstate(under='ignore'):
        P, _, _ = model_ref.adam_tf({'a': inp.p.copy()}, {'a': inp.m.copy()}, {'a': inp.v.copy()}, {'a': inp.g}, t=5)
    assert np.max(np.abs(out.inner('p') - P['a'])) < 1e-6


# ---------------------------------------------------------------------------------- cc_adam_dense_t
SHAPES6 = [(1, 4), (2, 130), (36, 2), (64, 64), (65, 68), (256, 130)]


def _place(items, tail):
    """[(gap before, (rows, cols))] -> (n, [(off, rows, cols)])."""
    off, out = 0, []
    for gap, (r, c) in items:
        off += gap
        out.append((off, r, c))
        off += r * c
    return off + tail, out


T_LAYOUTS = {
    # a region at offset 0, two with no gap between them ((2, 130) and (36, 2)), the last ending at n
    'six': _place(list(zip((0, 8, 0, 24, 100, 36), SHAPES6)), 0),
    'twelve': _place([(20 + 4 * i, s) for i, s in enumerate(SHAPES6 + SHAPES6[::-1])], 52),
    'none': (4100, []),
    'all': _place([(0, s) for s in SHAPES6], 0),                       # no flat blocks
    'stride': _place([(1000, (64, 64))], 2048 * 256 * 4 + 3096),       # the flat blocks' grid-stride loop iterates
}
assert T_LAYOUTS['stride'][0] - 64 * 64 > 2048 * 256 * 4 and len(T_LAYOUTS['twelve'][1]) == 12
assert all(n % 4 == 0 for n, _ in T_LAYOUTS.values())


def _dense_t(layout, regime, step, bpe):
    n, regs = T_LAYOUTS[layout]
    inp = AR.inputs(regime, n, probes=False)
    want = _dense(Bufs.of(inp), [(0, n)], step)
    got = Bufs.of(inp)
    dsts = [_guarded(np.full(r * c, FILL16, np.int16), np.int16(FILL16)) for _, r, c in regs]
    arr = (L.AdamTRegion * max(1, len(regs)))()
    for i, ((o, r, c), d) in enumerate(zip(regs, dsts)):
        arr[i].off, arr[i].rows, arr[i].cols, arr[i].dst = o, r, c, d.data_ptr() + 2 * GUARD
    st = _state(step, 2)
    _call('cc_adam_dense_t', *got.pmvgs(), n, L.ptr(st), *AR.HP_DEFAULT, arr if regs else None, len(regs), bpe,
          L.stream_ptr())
    torch.cuda.synchronize()
    tag = (layout, regime, step, bpe)
    assert got.same(want) == [], (tag, got.same(want))
    assert st.tolist() == ([step + 1, 0, 1, 0] if bpe else [step, 2, 0, 0]), tag
    sh = want.inner('s')
    for (o, r, c), d in zip(regs, dsts):
        d = d.cpu().numpy().view(np.uint16)
        assert np.all(d[:GUARD] == FILL16) and np.all(d[GUARD + r * c:] == FILL16), (tag, 'dst sentinel')
        assert np.array_equal(d[GUARD:GUARD + r * c].reshape(c, r), AR.transposed_region(sh, o, r, c)), (tag, o, r, c)


@pytest.mark.parametrize('bpe', [0, 3])
@pytest.mark.parametrize('layout', ['six', 'twelve', 'none', 'all'])
def test_adam_dense_t(layout, bpe):
    for regime in AR.FUSED_REGIMES:
        for step in AR.FUSED_STEPS:
            _dense_t(layout, regime, step, bpe)


def test_adam_dense_t_flat_grid_stride():
    _dense_t('stride', 'absent', 4, 3)


# ---------------------------------------------------------------------------------- cc_tower_bwd_chain_adam
_TOWER = {}


def _tower():
    """The existing case's tower: (a: cc_tower_bwd_chain's outputs, b: the Run the Adam variant writes)."""
    if not _TOWER:
        inp = TR.case_inputs(256, 32, 96, True)
        images = ('act6t', 'act6p', 'pt', 'gpre1p')
        a, b = Run(inp, True, images), Run(inp, True, images)
        a.call(*_CHAIN)
        b.call('cc_tower_transpose', 'cc_tower_fwd')
        # what the forward left at its prefill is the chain's to write
        chain = [k for k in b.out if bool((b.out[k] == FILL).all())]
        assert 'gpre1' in chain and 'gact0' in chain and 'act6' not in chain
        _TOWER['b'], _TOWER['want'] = b, {k: a.get(k).copy() for k in chain}
        assert not np.any(_TOWER['want']['gpre1'] == FILL)
    return _TOWER['b'], _TOWER['want']


def _chain_blocks(n, R=96):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, min(-(-(-(-n // 4)) // 2048), max(cus - R // 32, 8)))


def _chain_adam(lo0, n0, lo1, n1, regime, step, shadow=True):
    b, chain_want = _tower()
    n = max(lo0 + n0, lo1 + n1) + 9
    inp = AR.inputs(regime, n, probes=False)
    ranges = [(lo0, n0)] + ([(lo1, n1)] if n1 else [])
    want = _dense(Bufs.of(inp), ranges, step, shadow=shadow)
    got = Bufs.of(inp)
    st = _state(step)
    b.refill(*chain_want)
    _call('cc_tower_bwd_chain_adam', ctypes.byref(b.t), *got.pmvgs(0, shadow), lo0, n0, lo1, n1, L.ptr(st),
          *AR.HP_DEFAULT, L.stream_ptr())
    torch.cuda.synchronize()
    tag = (lo0, n0, lo1, n1, regime, step, shadow)
    assert got.same(want) == [], (tag, got.same(want))
    assert st.tolist() == [step, 1, 0, 0]
    assert all(np.array_equal(b.get(k), w) for k, w in chain_want.items()), (tag, 'the chain\'s outputs')


def _chain_big():
    """Ranges sized from the entry's own block count: every block makes a second pass of range_u<4>
    over range 0, and that pass ends after 1 or 2 of the thread's four float4 groups."""
    stride = None
    n0 = 2_500_000
    for _ in range(3):
        stride = _chain_blocks(n0 + 1001) * 512
        n0 = 4 * (5 * stride + stride // 2) + 3
    n4 = n0 // 4
    assert 4 * stride + stride <= n4 < 4 * stride + 2 * stride and _chain_blocks(n0 + 1001) * 512 == stride
    lo1 = 64 + (n0 + 3) // 4 * 4 + 8
    return 64, n0, lo1, 1001


CHAIN_SMALL = {'tail2_and_n1': (64, 1002, 2048, 4100, True), 'tail3_n1_zero': (64, 1003, 0, 0, True),
               'tail1_no_shadow': (64, 1001, 2048, 4103, False)}


@pytest.mark.parametrize('case', list(CHAIN_SMALL))
def test_tower_chain_adam_ranges(case):
    lo0, n0, lo1, n1, shadow = CHAIN_SMALL[case]
    for regime in AR.FUSED_REGIMES:
        for step in AR.FUSED_STEPS:
            _chain_adam(lo0, n0, lo1, n1, regime, step, shadow)


@pytest.mark.parametrize('regime', AR.FUSED_REGIMES)
def test_tower_chain_adam_second_pass(regime):
    lo0, n0, lo1, n1 = _chain_big()
    for step in AR.FUSED_STEPS:
        _chain_adam(lo0, n0, lo1, n1, regime, step)


# ---------------------------------------------------------------------------------- the W1-gradient epilogue
@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('R', [96, 544])
def test_embed_grad_cs_adam_forms(R, packed):
    """cc_embed_grad_cs_adam / _reg == cc_embed_grad_cs (+ the reg rows) then cc_adam_dense, at bits
    sparse enough that most W1 rows have no bit: their gradient is exactly 0 (the absent case)."""
    V, D, nreg = CS.V, CS.D, 64
    rng = np.random.default_rng(R + packed)
    gen, img, RP, xt_all, xt_cube, rid = CS._reg_problem(R, nreg, packed)
    # replace the dense bits of the helper's problem by sparse ones
    X = np.zeros((R + nreg, V), bool)
    X[:R] = rng.random((R, V)) < 1.0 - 0.9 ** (1.0 / R)
    ridh = rid.cpu().numpy()
    real = np.nonzero(ridh >= 0)[0]
    X[R + real, ridh[real]] = True
    xt_all, xt_cube = CS._bits(X), CS._bits(X[:R])
    img0, RP0 = CS._image(R, packed, gen)                 # the cube rows alone, as the existing Adam-form test has them
    grad, bg = CS._plain(img0, packed, R, RP0, xt_cube)
    grad_r, bg_r = CS._plain(img, packed, R + nreg, RP, xt_all)
    assert float((grad.abs().sum(1) == 0).float().mean()) > 0.5, 'most W1 rows should have a zero gradient'
    reg = (L.ptr(rid), nreg, R // 16)
    names = 'p m v shadow bias_grad'.split()

    def same(got, want):
        bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
        bad = [n for n, a, b in zip(names, got, want) if not torch.equal(bits(a), bits(b))]
        assert not bad, (regime, step, bad)
    for regime in AR.FUSED_REGIMES:
        inp = AR.inputs(regime, V * D, probes=False)
        pmv = tuple(torch.from_numpy(np.array(a)).cuda() for a in (inp.p, inp.m, inp.v))
        for step in AR.FUSED_STEPS:
            st = _state(step)
            CALLED.update(('cc_adam_dense', 'cc_embed_grad_cs_adam', 'cc_embed_grad_cs_adam_reg'))
            same(CS._adam_form(img0, packed, R, RP0, xt_cube, pmv, st), CS._adam_dense(grad, pmv, st) + (bg,))
            same(CS._adam_form(img, packed, R, RP, xt_cube, pmv, st, reg), CS._adam_dense(grad_r, pmv, st) + (bg_r,))
            assert st.tolist() == [step, 1, 0, 0]


# ---------------------------------------------------------------------------------- cc_to_bf16
@pytest.mark.parametrize('n', [1, 5, 10007])
def test_to_bf16_ties(n):
    x = AR.inputs('ties', n, probes=False).p
    dx = _guarded(np.array(x), np.float32(FILL))
    dy = _guarded(np.full(n, FILL16, np.int16), np.int16(FILL16))
    L.call('cc_to_bf16', dx.data_ptr() + 4 * GUARD, dy.data_ptr() + 2 * GUARD, n, L.stream_ptr())
    torch.cuda.synchronize()
    y = dy.cpu().numpy().view(np.uint16)
    assert np.all(y[:GUARD] == FILL16) and np.all(y[GUARD + n:] == FILL16)
    assert np.array_equal(y[GUARD:GUARD + n], AR.bf16_rne(x))


# ---------------------------------------------------------------------------------- refusals
def _off(ptr, nbytes):
    return ctypes.c_void_p(ptr.value + nbytes)


def test_refusals_and_empty_calls():
    """Every bad call returns nonzero and writes nothing; n = 0 returns OK and writes nothing."""
    lib, hp, s = L.lib(), AR.HP_DEFAULT, L.stream_ptr()
    n = 8192
    inp = AR.inputs('trained', n + 8, probes=False)
    clean, b = Bufs.of(inp), Bufs.of(inp)
    st = _state(4)
    P, M, V_, G, S = b.pmvgs()
    dst = torch.full((GUARD + 64 * 64 + GUARD,), FILL16, device='cuda', dtype=torch.int16)

    def regions(*items):
        arr = (L.AdamTRegion * len(items))()
        for i, (o, r, c) in enumerate(items):
            arr[i].off, arr[i].rows, arr[i].cols, arr[i].dst = o, r, c, dst.data_ptr() + 2 * GUARD
        return arr, len(items)

    tower512 = L.TowerArgs(dtype=L.CC_BF16, d=512, B=32, R=96)
    dense_t = lambda p=P, sh=S, n_=n, regs=(None, 0): lib.cc_adam_dense_t(p, M, V_, G, sh, n_, L.ptr(st), *hp, *regs, 0, s)
    bad = {
        'dense: p offset by one element': lambda: lib.cc_adam_dense(_off(P, 4), M, V_, G, S, n, L.ptr(st), *hp, s),
        'dense: shadow not 8-byte aligned': lambda: lib.cc_adam_dense(P, M, V_, G, _off(S, 2), n, L.ptr(st), *hp, s),
        'dense_t: p offset by one element': lambda: dense_t(p=_off(P, 4)),
        'dense_t: shadow not 8-byte aligned': lambda: dense_t(sh=_off(S, 2)),
        'dense_t: n % 4': lambda: dense_t(n_=n + 2),
        'dense_t: unsorted': lambda: dense_t(regs=regions((4096, 8, 8), (0, 8, 8))),
        'dense_t: overlapping': lambda: dense_t(regs=regions((0, 8, 8), (60, 8, 8))),
        'dense_t: past n': lambda: dense_t(regs=regions((n - 60, 8, 8))),
        'dense_t: thirteen regions': lambda: dense_t(regs=regions(*[(64 * i, 8, 8) for i in range(13)])),
        'chain: d = 512': lambda: lib.cc_tower_bwd_chain_adam(ctypes.byref(tower512), P, M, V_, G, S, 0, n, 0, 0, L.ptr(st),
                                                              *hp, s),
    }
    for what, fn in bad.items():
        assert fn() != 0, f'{what}: accepted'
    torch.cuda.synchronize()
    # n = 0: OK, nothing written
    assert lib.cc_adam_dense(P, M, V_, G, S, 0, L.ptr(st), *hp, s) == 0
    assert lib.cc_adam_dense_t(P, M, V_, G, S, 0, L.ptr(st), *hp, None, 0, 3, s) == 0
    b2, _ = _tower()
    assert lib.cc_tower_bwd_chain_adam(ctypes.byref(b2.t), P, M, V_, G, S, 0, 0, 0, 0, L.ptr(st), *hp, s) == 0
    torch.cuda.synchronize()
    assert b.same(clean) == [] and bool((dst == FILL16).all())
    assert st.tolist() == [4, 1, 0, 0]


def test_every_entry_was_exercised(request):
    """Runs last: every entry of ENTRIES was called by this file (checked when the whole file ran)."""
    mine = {i.originalname for i in request.session.items if i.path == request.node.path}
    if mine >= {n for n in dir(request.module) if n.startswith('test_')}:
        assert ENTRIES <= CALLED, sorted(ENTRIES - CALLED)
