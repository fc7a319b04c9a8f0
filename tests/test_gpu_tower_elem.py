"""The fused tower kernels (csrc/tower.hip) against fp64, per element and per layer, at the smallest
shapes that reach every kernel family, template instantiation and branch (run on an MI355X).

Reference principle (tests/tower_ref.py; tests/test_tower_ref_host.py holds it to torch autograd):
every layer is checked by itself, in fp64, from the inputs of that layer AS THE GPU STORED THEM, so
exactly one rounding step of the kernel separates it from the reference — no bound has to absorb
six layers of compounded bf16 rounding, as the Frobenius bar of test_gpu_tower.py does.  Chain
layers i = 0..5 have K_i, N_i of chain_dims; rows [0, B) use weights l = i, rows [B, R) l = i + 3
for i >= 3, and W_l, b_l differ between the two decoder branches, so a block that picks the wrong
branch is loud.  The bounds are derived, not tuned (u = 2^-24):
  fwd    ref = relu(act[i] W_l + b_l);  eps = (K_i + 4) u (|act[i]| |W_l| + |b_l|): fp32 accumulation
         in any order (bf16 products are exact in fp32; + 4: the fp32 operand path's product
         roundings and the bias add).  |act[i+1] - ref| <= 2^-8 (ref + eps) + eps in bf16 (one bf16
         rounding of the fp32 value, the repo's conservative 2^-8 as in test_gpu_decreg.py), eps in
         fp32.  relu is 1-Lipschitz: elements near zero need no special case
  bwd    ref = (G_i W_l^T) * (act[i] > 0), G_5 = gD3, G_i = the kernel's own gact[i], the mask from the
         kernel's own act[i];  eps = (N_i + 4) u |G_i| |W_l^T|.  |gact[i-1] - ref| <= 2^-8 (|ref| +
         eps) + eps (bf16) or eps (fp32); masked elements are bit-zero
  gpre1  layer 0's dX, fp32 in both formats: eps
  gw,gb  gw_l = H^T G, gb_l = colsum G over the layer's rows (all R for l < 3, [0, B) for l = 3..5,
         [B, R) for l = 6..8) of the kernel's own stored H_i, G_i: no bf16 rounding at all, only fp32
         accumulation: (rows + 2) u |H|^T |G| and (rows + 2) u colsum |G| (fp32 operands: rows + 4)
  images act6t = act[6]^T; act6p, act6tp, hpt[i] (= act[i]) and gpt[i] (= G_i) in the fragment layouts
         of include/ccrec.h; gpre1t [d][ceil64(R)] and gpre1p (reduction ceil64(R)) = f2bf of the
         kernel's own fp32 gpre1: all BIT-EXACT rearrangements of what the same launch stored as
         rows; columns / fragment rows R .. ceil64(R) keep the prefill byte for byte
Every output is prefilled with FILL between GUARD untouched elements on either side; with R == B
layers 6..8 are null pointers (the kernels touch none of their buffers).  The inputs keep every
layer's share of positive pre-activations within [0.3, 0.7] (asserted on the host): a mask test on
rows that are all live, or all dead, checks nothing.

Largest observed error / bound per check and kernel family over all cases (MI355X; the per-case
values go to $CCREC_PARITY_LOG through gpu_helpers.record_errors):
                 fwd     bwd     gpre1
  generic fp32   0.052   0.049   0.015
  generic bf16   0.987   0.993   0.0072
  fast           0.993   0.989   0.0053
  wide           0.992   0.993   0.0064
                 gw      gb
  slab fp32      0.084   0.057
  slab bf16      0.040   0.0066
  tiled          0.040   0.0066
  packed         0.040   0.0066   (one wave over the 3,104 rows: 0.037, 3.6e-5)
  split          0.037   2.9e-5
A ratio above 1 is a finding about the kernel.  In bf16, fwd and bwd sit at 0.97 .. 0.99 in every
case: half an ulp of bf16 IS 2^-8 relative just above a power of two, and among some 10^4 elements
one lands there, so the bound is the rounding's own and a kernel that truncated instead of rounding
to nearest would double it.  Bounds with slack (largest ratio below 0.01): gpre1 in the three bf16
families, and gb on every bf16 path — both are worst-case linear bounds (N_i + 4, rows + 2 terms
all rounding the same way) of errors that grow like the square root of the term count (gb at
3,104 rows: 3e-5).  They are kept as derived: they still fail on one dropped 16-row step or one
flipped mask element
(test_tower_ref_host.py), which is the fault they are there to catch.  The fp32 rows and gw (0.04,
the figure of test_gpu_decreg.py's gwk bound of the same form) have the same kind of slack, above
0.01.
"""
import ctypes

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from tests import tower_ref as TR
from tests.gpu_helpers import record_errors

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 7.0           # exact in bf16 (0x40E0) and fp32


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    L.lib()


def _np(t):
    """A device tensor as numpy: bf16 as uint16 bit patterns, fp32 as float32."""
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


class Run:
    """One set of tower buffers.  Inputs are plain tensors; every output is FILL with GUARD elements
    on either side of the region the kernels own (get() asserts the guards and returns the region)."""

    def __init__(self, inp, packed_w=False, images=()):
        d, B, R = inp.d, inp.B, inp.R
        self.inp, self.images = inp, set(images)
        self.tdt = torch.bfloat16 if inp.bf16 else torch.float32
        self.nl = 9 if R > B else 6
        self.t = t = L.TowerArgs(dtype=L.CC_BF16 if inp.bf16 else L.CC_F32, d=d, B=B, R=R)
        self.keep, self.out = [], {}
        dims, w = TR.chain_dims(d), TR.widths(d)
        dev = lambda a, dt=self.tdt: self._hold(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to('cuda', dt))
        zeros = lambda n: self._hold(torch.zeros(n, device='cuda', dtype=self.tdt))
        for l in range(self.nl):     # R == B: layers 6..8 stay null
            t.w[l], t.b[l] = dev(inp.W[l]).data_ptr(), dev(inp.b[l], torch.float32).data_ptr()
            t.wt[l] = zeros(inp.W[l].size).data_ptr()
            if packed_w:
                t.wpf[l], t.wpb[l] = zeros(inp.W[l].size).data_ptr(), zeros(inp.W[l].size).data_ptr()
            t.gw[l], t.gb[l] = self._guarded(f'gw{l}', inp.W[l].size, torch.float32), self._guarded(f'gb{l}', dims[l if l < 6 else l - 3][1], torch.float32)
        t.act[0], t.gD3 = dev(inp.x0).data_ptr(), dev(inp.gD3).data_ptr()
        for a in range(1, 7):
            t.act[a] = self._guarded(f'act{a}', R * w[a])
        for a in range(5):
            t.gact[a] = self._guarded(f'gact{a}', R * w[a + 1])
        t.gpre1 = self._guarded('gpre1', R * d, torch.float32)
        self.slab = self._hold(torch.zeros((R // 32) * int(L.lib().cc_tower_slab_elems(d)), device='cuda'))
        t.slab = self.slab.data_ptr()
        r64 = TR.ceil64(R)
        if 'act6t' in self.images:
            t.act6t = self._guarded('act6t', d * R)
        if 'act6p' in self.images:
            t.act6p, t.act6tp = self._guarded('act6p', R * d), self._guarded('act6tp', R * d)
        if 'pt' in self.images:
            for i, (K, N) in enumerate(dims):
                t.hpt[i], t.gpt[i] = self._guarded(f'hpt{i}', R * K), self._guarded(f'gpt{i}', R * N)
        if 'gpre1t' in self.images:
            t.gpre1t = self._guarded('gpre1t', d * r64)
        if 'gpre1p' in self.images:
            t.gpre1p = self._guarded('gpre1p', d * r64)

    def _hold(self, x):
        self.keep.append(x)
        return x

    def _guarded(self, name, n, dt=None):
        buf = torch.full((GUARD + n + GUARD,), FILL, device='cuda', dtype=dt or self.tdt)
        self.out[name] = buf
        return buf.data_ptr() + GUARD * buf.element_size()

    def call(self, *fns):
        for fn in fns:
            L.call(fn, ctypes.byref(self.t), L.stream_ptr())
        torch.cuda.synchronize()

    def refill(self, *names):
        for n in names:
            self.out[n].fill_(FILL)

    def get(self, name):
        buf = self.out[name]
        assert torch.all(buf[:GUARD] == FILL) and torch.all(buf[-GUARD:] == FILL), f'{name}: guard overwritten'
        return _np(buf[GUARD:-GUARD])

    def val(self, name, cols):
        """An output as fp64 [rows][cols]."""
        a = self.get(name)
        return (TR.from_bits(a) if a.dtype == np.uint16 else a.astype(np.float64)).reshape(-1, cols)

    def stored(self):
        """(act[0..6], G_0..G_5) as the kernels stored them, fp64."""
        w = TR.widths(self.inp.d)
        acts = [self.inp.x0] + [self.val(f'act{a}', w[a]) for a in range(1, 7)]
        Gs = [self.val(f'gact{a}', w[a + 1]) for a in range(5)] + [self.inp.gD3]
        return acts, Gs


_FILL_BITS = int(TR.bits(np.array([FILL], np.float32))[0])


def _check_chain(run, errs):
    """Forward, backward and gpre1 per element and layer; then every image of the run, bitwise."""
    inp = run.inp
    d, R, bf16 = inp.d, inp.R, inp.bf16
    w = TR.widths(d)
    acts, Gs = run.stored()
    fwd, bwd = [], []
    for i in range(6):
        ref, eps = TR.fwd_layer(inp, i, acts[i])
        fwd.append(TR.ratio(np.abs(acts[i + 1] - ref), TR.stored_bound(ref, eps, bf16)))
    for i in range(5, -1, -1):
        ref, eps, mask = TR.bwd_layer(inp, i, Gs[i], acts[i])
        assert 0.2 < mask.mean() < 0.8, (i, mask.mean())       # the kernel's own mask is mixed too
        raw = run.get(f'gact{i - 1}' if i else 'gpre1').reshape(R, w[i])
        assert np.all(raw.view(np.uint16 if raw.dtype == np.uint16 else np.uint32)[~mask] == 0), f'layer {i}: masked element not bit-zero'
        got = Gs[i - 1] if i else raw.astype(np.float64)
        r = TR.ratio(np.abs(got - ref), TR.stored_bound(ref, eps, bf16 and i > 0) * mask)
        if i:
            bwd.append(r)
        else:
            errs['gpre1'] = r
    errs['fwd'], errs['bwd'] = max(fwd), max(bwd)
    errs.update({f'fwd{i}': v for i, v in enumerate(fwd)})
    errs.update({f'bwd{5 - k}': v for k, v in enumerate(bwd)})
    # images: bit-exact rearrangements of the rows of the same launch
    D3 = run.get('act6').reshape(R, d)
    r64 = TR.ceil64(R)
    if 'act6t' in run.images:
        assert np.array_equal(run.get('act6t').reshape(d, R), D3.T), 'act6t'
    if 'act6p' in run.images:
        assert np.array_equal(run.get('act6p'), TR.pack_rows(D3)), 'act6p'
        assert np.array_equal(run.get('act6tp'), TR.pack_t(D3)), 'act6tp'
    if 'pt' in run.images:
        _check_pt(run)
    if 'gpre1t' in run.images or 'gpre1p' in run.images:
        gb = TR.bits(run.get('gpre1')).reshape(R, d)       # f2bf of the kernel's own fp32 gpre1
        if 'gpre1t' in run.images:
            assert np.array_equal(run.get('gpre1t').reshape(d, r64), TR.transpose_ld(gb, r64, _FILL_BITS)), 'gpre1t'
        if 'gpre1p' in run.images:
            assert np.array_equal(run.get('gpre1p'), TR.pack_t(gb, r64, _FILL_BITS)), 'gpre1p'


def _check_pt(run):
    """hpt[i] = act[i] and gpt[i] = G_i, packed transposed, bit for bit."""
    inp = run.inp
    w = TR.widths(inp.d)
    for i in range(6):
        H = TR.bits(inp.x0) if i == 0 else run.get(f'act{i}').reshape(inp.R, w[i])
        G = TR.bits(inp.gD3) if i == 5 else run.get(f'gact{i}').reshape(inp.R, w[i + 1])
        assert np.array_equal(run.get(f'hpt{i}'), TR.pack_t(H)), f'hpt{i}'
        assert np.array_equal(run.get(f'gpt{i}'), TR.pack_t(G)), f'gpt{i}'


def _check_dw(run, errs):
    """gw / gb of every layer against H^T G, colsum G of the kernel's own stored H_i, G_i."""
    acts, Gs = run.stored()
    gw, gb = [], []
    for l in range(run.nl):
        K, N = run.inp.W[l].shape
        rw, bw, rb, bb = TR.dw_layer(run.inp, l, acts, Gs)
        gw.append(TR.ratio(np.abs(run.val(f'gw{l}', N) - rw), bw))
        gb.append(TR.ratio(np.abs(run.val(f'gb{l}', N)[0] - rb), bb))
    errs['gw'], errs['gb'] = max(gw), max(gb)
    errs.update({f'gw{l}': v for l, v in enumerate(gw)})
    errs.update({f'gb{l}': v for l, v in enumerate(gb)})


def _finish(request, errs, keys):
    print(request.node.name, errs)
    record_errors(request.node.name, 0, errs)
    bad = {k: errs[k] for k in keys if not errs[k] <= 1}
    assert not bad, bad


_CHAIN = ('cc_tower_transpose', 'cc_tower_fwd', 'cc_tower_bwd_chain')

# family, (d, B, R, bf16), packed weight images, images
CHAIN_CASES = (
    [('generic_f32', s, False, ('act6t',)) for s in TR.SHAPES['generic_f32']]
    + [('generic_bf16', s, False, ('act6t', 'gpre1t')) for s in TR.SHAPES['generic_bf16']]
    + [('fast', s, pk, ('act6t', 'act6p', 'pt', 'gpre1p' if pk else 'gpre1t'))
       for s in TR.SHAPES['fast'] for pk in (False, True)]
    + [('wide', s, True, ('act6t', 'act6p', 'pt', 'gpre1t')) for s in TR.SHAPES['wide']])


@pytest.mark.parametrize('family,shape,packed_w,images', [
    pytest.param(f, s, pk, im, id=f'{f}-d{s[0]}-B{s[1]}-R{s[2]}-{"wp" if pk else "w"}') for f, s, pk, im in CHAIN_CASES])
def test_tower_chain_elementwise(request, family, shape, packed_w, images):
    """cc_tower_fwd and cc_tower_bwd_chain: every stored element of every layer (module docstring)."""
    run = Run(TR.case_inputs(*shape), packed_w, images)
    run.call(*_CHAIN)
    errs = {}
    _check_chain(run, errs)
    _finish(request, errs, ('fwd', 'bwd', 'gpre1'))


def test_tower_slab_dw(request):
    """cc_tower_bwd_dw + cc_tower_reduce (per-block slabs, summed in block order)."""
    for name, shape in (('slab_f32', (64, 32, 96, False)), ('slab_bf16', (256, 32, 96, True))):
        run = Run(TR.case_inputs(*shape))
        run.call(*_CHAIN, 'cc_tower_bwd_dw', 'cc_tower_reduce')
        errs = {}
        _check_dw(run, errs)
        _finish(request, {f'{name}_{k}': v for k, v in errs.items()}, (f'{name}_gw', f'{name}_gb'))


@pytest.mark.parametrize('d,B,R', [(256, 32, 96), (64, 64, 64)])
def test_tower_tiled_dw(request, d, B, R):
    """cc_tower_bwd_dw_direct without hpt / gpt: the LDS-staged tiled kernel.  (256, 32, 96): 32 rows
    per wave, so the B-row decoder layers leave three waves with all-zero rows."""
    run = Run(TR.case_inputs(d, B, R, True), packed_w=True)
    run.call(*_CHAIN, 'cc_tower_bwd_dw_direct')
    errs = {}
    _check_dw(run, errs)
    _finish(request, errs, ('gw', 'gb'))


@pytest.mark.parametrize('d,B,R', [(256, 32, 96), (128, 32, 160)])
def test_tower_packed_dw(request, d, B, R):
    """cc_tower_bwd_dw_direct from hpt / gpt: one wave per tile.  (256, 32, 96): 6, 2 and 4 sixteen-row
    steps (the tail loop only); (128, 32, 160): 10 = one unrolled batch of 8 and a tail of 2."""
    run = Run(TR.case_inputs(d, B, R, True), packed_w=True, images=('pt',))
    run.call(*_CHAIN, 'cc_tower_bwd_dw_direct')
    _check_pt(run)
    errs = {}
    _check_dw(run, errs)
    _finish(request, errs, ('gw', 'gb'))


def test_tower_split_dw(request):
    """R = 3104 >= 2048: the row-split kernels (S = 3; the encoder's 194 sixteen-row steps split
    65 / 65 / 64, the cube decoder's 2 steps leave split 2 with no rows) and, with slab = NULL, the
    one-wave chain over all 3,104 rows: the same bound for both."""
    run = Run(TR.case_inputs(64, 32, 3104, True), packed_w=True, images=('pt',))
    run.call(*_CHAIN, 'cc_tower_bwd_dw_direct')
    _check_pt(run)
    errs, one = {}, {}
    _check_dw(run, errs)
    names = [f'g{k}{l}' for k in 'wb' for l in range(9)]
    split = {n: run.get(n).copy() for n in names}
    run.refill(*names)
    run.t.slab = None
    run.call('cc_tower_bwd_dw_direct')
    _check_dw(run, one)
    errs.update({f'packed_{k}': v for k, v in one.items()})
    assert any(not np.array_equal(split[n], run.get(n)) for n in names), 'slab = NULL did not change the kernel'
    _finish(request, errs, ('gw', 'gb', 'packed_gw', 'packed_gb'))


def test_tower_chain_adam_blocks():
    """cc_tower_bwd_chain_adam: the chain's outputs are those of cc_tower_bwd_chain bit for bit; p, m,
    v and the shadow are cc_adam_dense's over the two ranges and untouched everywhere else."""
    inp = TR.case_inputs(256, 32, 96, True)
    images = ('act6t', 'act6p', 'pt', 'gpre1p')
    a, b = Run(inp, True, images), Run(inp, True, images)
    a.call(*_CHAIN)
    n, lo0, n0, lo1, n1 = 8192, 64, 1002, 2048, 4100      # n0: a 2-element tail after the float4 body
    rng = np.random.default_rng(5)
    f = lambda x: torch.from_numpy(x.astype(np.float32)).cuda()
    p0, m0, g = f(rng.standard_normal(n)), f(rng.standard_normal(n) * 0.1), f(rng.standard_normal(n))
    v0 = f(rng.random(n) * 0.01)
    s0 = torch.full((n,), FILL, device='cuda', dtype=torch.bfloat16)
    state = torch.tensor([3, 1, 0, 0], device='cuda', dtype=torch.int64)
    hp = (1e-3, 0.9, 0.999, 1e-7)
    ref = [x.clone() for x in (p0, m0, v0, s0)]
    for lo, cnt in ((lo0, n0), (lo1, n1)):
        L.call('cc_adam_dense', *(x.data_ptr() + lo * x.element_size() for x in ref[:3]), g.data_ptr() + 4 * lo,
               ref[3].data_ptr() + 2 * lo, cnt, L.ptr(state), *hp, L.stream_ptr())
    got = [x.clone() for x in (p0, m0, v0, s0)]
    b.call('cc_tower_transpose', 'cc_tower_fwd')
    L.call('cc_tower_bwd_chain_adam', ctypes.byref(b.t), *(L.ptr(x) for x in got[:3]), L.ptr(g), L.ptr(got[3]),
           lo0, n0, lo1, n1, L.ptr(state), *hp, L.stream_ptr())
    torch.cuda.synchronize()
    for name in a.out:
        assert np.array_equal(a.get(name), b.get(name)), name
    assert not np.any(a.get('gpre1') == FILL)
    inside = np.zeros(n, bool)
    inside[lo0:lo0 + n0] = inside[lo1:lo1 + n1] = True
    for x, r, o in zip(got, ref, (p0, m0, v0, s0)):
        x, r, o = _np(x), _np(r), _np(o)
        assert np.array_equal(x, r)
        assert np.array_equal(x[~inside], o[~inside]) and np.mean(x[inside] != o[inside]) > 0.99
    assert state.tolist() == [3, 1, 0, 0]
