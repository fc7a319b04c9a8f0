"""cc_dec_softmax_kl_dw (decreg.hip, the fused D2 output layer) and cc_kl_tsum against fp64, per
element, at the smallest shapes that reach every branch of the host entry (run on an MI355X).

The reference is fp64 on the same bf16-rounded operands (gpu_helpers._softmax_kl_ref).  The bounds
are derived, not tuned (mag = scale (p S + t), S = sum_j t, bounds every intermediate the kernel
rounds):
  dz   |dZ - dz_ref| <= 2^-7 mag per element of every live row.  The kernel rounds dZ to bf16 (8
       significant bits: 2^-8 relative per rounding) twice at most: the main value, and the in-place
       sum with the clip correction (formed in fp32); + the fp32 softmax's ~1e-5.  |dz| <= mag before
       and after the correction, so two roundings reach 2^-7 mag only where both fall at the very
       edge of their half-ulp on an element with t << p S
  gw   |gW - D3^T dz_ref| <= 2^-7 |D3|^T mag,  gb  |gb - colsum dz_ref| <= 2^-7 colsum mag
  gwk  (clip-free) |gW - D3^T dZ_kernel| <= (rows + 2) 2^-24 |D3|^T |dZ_kernel|: fp32 accumulation
       in any order, kl_dwo2's two halves included — separates a dWo bug from a dZ bug
  loss relative 5e-6 (the bound of test_full_mode_clip_fix_path)
  tsum (V + 2) 2^-24 against sum |t| and sum |t ln t|
Padding rows (reg_idx = -1): the kernel WRITES their dZ rows as zeros (bit-zero over the prefill),
and they add nothing to dWo, dbo or the loss.

Largest observed error / bound per check over all cases (MI355X; the per-case values go to
$CCREC_PARITY_LOG through gpu_helpers.record_errors):
              dz      gw      gb       gwk     loss    loss_part
  clip-free   0.498   0.297   5.6e-5   0.042   0.064   0
  clip-live   0.912   0.431   0.206    -       0.093   0
  cc_kl_tsum  sum t 0.065, sum t ln t 0.836 (both at V = 1: one term, the fast log's own error)
A ratio above 1 is a finding about the kernel.  Clip-free, dz sits at 0.5 (its one bf16 rounding
at full half-ulp on some element) and gb at 5e-5 (dbo sums the fp32 dz before its rounding); gwk is
a worst-case bound of an error that grows like sqrt(rows).  In the clip-live cases dz uses most of
its bound (two roundings), and no ratio of dz, gw or gb fell below 0.01 (smallest: dz 0.60,
gw 0.063, gb 0.018), so none of those bounds has slack to tighten.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from tests.gpu_helpers import _softmax_kl_ref, record_errors

pytestmark = pytest.mark.gpu

N_CARDS = 37
GUARD = 64
FILL = 7.0


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    L.lib()


Shape = namedtuple('Shape', 'rows d V row0 ldt mt_lo')
Inputs = namedtuple('Inputs', 'shape clip D3 Wo bo Mt reg_idx scale loss_scale')


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


@functools.lru_cache(maxsize=4)
def _inputs(shape, clip, seed):
    """The operands of one call (host tensors, rounded to the kernel's formats)."""
    rows, d, V, row0, ldt, mt_lo = shape
    rng = np.random.default_rng(seed)
    D3 = np.full((ldt, d), 100.0)              # rows outside row0 .. row0 + rows: loud if read
    D3[row0:row0 + rows] = rng.standard_normal((rows, d)) * 0.5
    Wo = rng.standard_normal((d, V)) * (1.6 / np.sqrt(d))   # logits of std ~0.8 at every d
    bo = (rng.standard_normal(V) * 0.1).astype(np.float32)
    if clip:                                   # p far below the 1e-7 clip on 30 % of the columns
        bo[rng.permutation(V)[:round(0.3 * V)]] -= 40.0
    Mt = rng.random((N_CARDS, V)) ** 8
    Mt /= Mt.sum(1, keepdims=True)
    Mt[:, ::7] = 0.0
    reg_idx = rng.integers(mt_lo, N_CARDS, rows).astype(np.int32)
    reg_idx[rows - 20:] = -1                   # the capacity round-up at the end of the range
    if rows >= 96:                             # one whole 32-row group in the middle
        g = rows // 32 // 2
        reg_idx[32 * g:32 * g + 32] = -1
    reg_idx[rng.choice(np.flatnonzero(reg_idx >= 0), 5, replace=False)] = -1    # scattered single rows
    return Inputs(shape, clip, _bf16(D3), _bf16(Wo), torch.from_numpy(bo), torch.from_numpy(Mt.astype(np.float32)),
                  torch.from_numpy(reg_idx), float(np.float32(0.3 / rows)), 1.0 / rows)


Ref = namedtuple('Ref', 'live p t kl dz mag D3r')


def _reference(inp):
    """fp64 on the same rounded operands; padding rows contribute nothing."""
    rows, d, V, row0, ldt, mt_lo = inp.shape
    D3r = inp.D3[row0:row0 + rows].double().numpy()
    z = D3r @ inp.Wo.double().numpy() + inp.bo.double().numpy()
    idx = inp.reg_idx.numpy()
    live = idx >= 0
    T = inp.Mt.numpy()[np.maximum(idx, 0)]
    kl, dz = _softmax_kl_ref(z, T, inp.scale, 1)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    t = np.clip(T.astype(np.float64), 1e-7, 1.0)
    mag = inp.scale * (p * t.sum(1, keepdims=True) + t)
    kl[~live], dz[~live], mag[~live] = 0.0, 0.0, 0.0
    return Ref(live, p, t, kl, dz, mag, D3r)


class State:
    """What a caller keeps between calls: the workspace, the loss partials and the ticket."""

    def __init__(self, shape):
        n = int(L.lib().cc_dec_kl_ws_size(shape.rows, shape.V))
        self.ws = torch.zeros(n, device='cuda', dtype=torch.uint8)
        self.part = torch.full((int(L.lib().cc_dec_kl_blocks(shape.V)),), FILL, device='cuda', dtype=torch.float64)
        self.ticket = torch.zeros(1, device='cuda', dtype=torch.int32)


Out = namedtuple('Out', 'dzbuf gWbuf gbbuf loss part ticket dz_off')


def _run(inp, flags=0, dz_off=0, mt_lo=None, state=None, with_loss=True):
    """One cc_dec_softmax_kl_dw call.  dZ, gW and gb are prefilled with FILL and carry GUARD
    elements on either side of the region the kernel owns; only cards mt_lo .. N_CARDS of M~ (and
    of its row constants) are resident, the pointers shifted as the trainer shifts them."""
    rows, d, V, row0, ldt, _ = inp.shape
    mt_lo = inp.shape.mt_lo if mt_lo is None else mt_lo
    state = state or State(inp.shape)
    R = row0 + rows
    D3p = inp.D3[:R].view(R // 32, 32, d // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().cuda()
    D3tp = inp.D3.t().contiguous().view(d // 32, 32, ldt // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().cuda()
    Wo, bo, idx = inp.Wo.cuda(), inp.bo.cuda(), inp.reg_idx.cuda()
    Mres = inp.Mt[mt_lo:].contiguous().cuda()
    tsum = torch.zeros(N_CARDS - mt_lo, 2, device='cuda')
    L.call('cc_kl_tsum', L.ptr(Mres), N_CARDS - mt_lo, V, L.ptr(tsum), L.stream_ptr())
    dzbuf = torch.full((GUARD + dz_off + rows * V + GUARD,), FILL, device='cuda', dtype=torch.bfloat16)
    gWbuf = torch.full((GUARD + d * V + GUARD,), FILL, device='cuda')
    gbbuf = torch.full((GUARD + V + GUARD,), FILL, device='cuda')
    loss = torch.full((1,), FILL, device='cuda', dtype=torch.float64)
    ka = L.DecKlArgs(d=d, V=V, rows=rows, ldt=ldt, row0=row0, D3p=D3p.data_ptr(), D3tp=D3tp.data_ptr(),
                     Wo=Wo.data_ptr(), bo=bo.data_ptr(), Mt=Mres.data_ptr() - mt_lo * V * 4,
                     tsum=tsum.data_ptr() - mt_lo * 8, mt_bytes=N_CARDS * V * 4, mt_lo=mt_lo, reg_idx=idx.data_ptr(),
                     scale=inp.scale, dZ=dzbuf.data_ptr() + 2 * (GUARD + dz_off), gW=gWbuf.data_ptr() + 4 * GUARD,
                     gb=gbbuf.data_ptr() + 4 * GUARD, loss_partials=state.part.data_ptr(),
                     loss_out=loss.data_ptr() if with_loss else None, loss_scale=inp.loss_scale,
                     ticket=state.ticket.data_ptr() if with_loss else None, ws=state.ws.data_ptr(), flags=flags)
    L.call('cc_dec_softmax_kl_dw', ctypes.byref(ka), L.stream_ptr())
    torch.cuda.synchronize()
    return Out(dzbuf.cpu(), gWbuf.cpu(), gbbuf.cpu(), loss.cpu(), state.part.cpu(), state.ticket.cpu(), dz_off)


def _same(a, b, loss=True):
    """Bit-identical outputs (guards included)."""
    ok = (torch.equal(a.dzbuf.view(torch.int16), b.dzbuf.view(torch.int16)) and torch.equal(a.gWbuf, b.gWbuf)
          and torch.equal(a.gbbuf, b.gbbuf) and torch.equal(a.part, b.part))
    return ok and (not loss or torch.equal(a.loss, b.loss))


def _ratio(err, bound):
    """max err / bound; where the bound is zero the error must be."""
    zero = bound == 0
    assert np.all(err[zero] == 0)
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


# rows, d, V, row0, ldt, mt_lo | flags, dZ element offset, clip settings | the branch the host entry picks
_T = [
    ((32, 128, 40, 0, 32, 0), 0, 0, (0, 1), 'one_partial_slice_one_row_group'),
    ((288, 256, 192, 64, 368, 0), 0, 0, (0, 1), 'two_exact_slices_rows_not_256n'),
    ((512, 256, 1001, 128, 640, 5), 0, 0, (0, 1), 'full_tile_odd_V_41col_tail_mtlo5'),
    ((96, 512, 200, 0, 96, 0), 0, 0, (0, 1), '64col_slices_vector_Wo_load'),
    ((544, 256, 1001, 32, 592, 0), 0, 0, (0, 1), 'two_tiles_odd_V_dWo_in_block'),
    ((544, 128, 1001, 0, 544, 5), 0, 0, (0, 1), 'two_tiles_odd_V_dWo_in_block_mtlo5'),
    ((544, 512, 999, 0, 544, 0), 0, 0, (0, 1), 'two_tiles_odd_V_dWo_in_block'),
    ((1056, 256, 1002, 64, 1120, 0), 0, 0, (0, 1), 'stats2_sep_dwo_256_false_no_16B_stores'),
    ((1056, 256, 1000, 64, 1120, 5), 0, 0, (0, 1), 'stats2_odd_slices_16B_stores_dwo2_40col_tail_mtlo5'),
    ((1056, 256, 1152, 0, 1056, 0), 0, 0, (1,), 'stats2_even_slices_dwo2_exact_slices'),
    ((1056, 256, 1000, 64, 1120, 5), L.CC_KL_DWO_NARROW, 0, (0, 1), 'narrow_flag_dwo_256_true'),
    ((544, 128, 1000, 0, 544, 0), 0, 0, (0, 1), 'dwo_128_true_16B_stores'),
    ((544, 512, 1000, 32, 592, 0), 0, 0, (0, 1), 'dwo_512_true_grid_y2'),
    ((544, 128, 1002, 0, 544, 0), 0, 0, (1,), 'dwo_128_false'),
    ((544, 512, 1002, 0, 544, 0), 0, 0, (1,), 'dwo_512_false'),
    ((1056, 256, 1000, 64, 1120, 0), 0, 2, (1,), 'dZ_unaligned_fallback_from_wstore_and_dwo2'),
]
CASES = [pytest.param(Shape(*s), fl, off, clip, 100 + 2 * i + clip,
                      id=f'r{s[0]}-d{s[1]}-V{s[2]}-{name}-clip{clip}')
         for i, (s, fl, off, clips, name) in enumerate(_T) for clip in clips]


@pytest.mark.parametrize('shape,flags,dz_off,clip,seed', CASES)
def test_dec_kl_elementwise(request, shape, flags, dz_off, clip, seed):
    """Every output element of one call against the fp64 reference (module docstring: the bounds)."""
    rows, d, V, row0, ldt, mt_lo = shape
    inp = _inputs(shape, clip, seed)
    ref = _reference(inp)
    live = ref.live
    # 1. the clip gap — a condition on the inputs: the kernel's fp32 p and the reference's fp64 p
    # fall on the same side of 1e-7 everywhere, so no element is left out of any comparison
    assert not np.any((ref.p >= 1e-8) & (ref.p <= 1e-6)), 'an input with p near the clip: change the seed'
    dead = ref.p < 1e-7
    if clip:   # the fix path does real work on every live row
        assert np.all((ref.t * dead).sum(1)[live] > 0.1)
    else:
        assert not dead.any()
    o = _run(inp, flags=flags, dz_off=dz_off)
    lo = GUARD + dz_off
    dzk_t = o.dzbuf[lo:lo + rows * V].view(rows, V)
    dzk = dzk_t.double().numpy()
    gW = o.gWbuf[GUARD:GUARD + d * V].view(d, V).double().numpy()
    gb = o.gbbuf[GUARD:GUARD + V].double().numpy()
    errs = {}
    # 2. dZ per element; padding rows are written as zeros
    errs['dz'] = _ratio(np.abs(dzk - ref.dz)[live], 2.0 ** -7 * ref.mag[live])
    assert np.all(dzk_t.view(torch.int16).numpy()[~live] == 0)
    # 3. dWo and dbo per element
    aD3 = np.abs(ref.D3r)
    errs['gw'] = _ratio(np.abs(gW - ref.D3r.T @ ref.dz), 2.0 ** -7 * (aD3.T @ ref.mag))
    errs['gb'] = _ratio(np.abs(gb - ref.dz.sum(0)), 2.0 ** -7 * ref.mag.sum(0))
    if not clip:
        errs['gwk'] = _ratio(np.abs(gW - ref.D3r.T @ dzk), (rows + 2) * 2.0 ** -24 * (aD3.T @ np.abs(dzk)))
    # 4. the loss
    want = ref.kl[live].sum() * inp.loss_scale
    nsl = -(-V // (96 if d <= 256 else 64))
    part = o.part.numpy()
    errs['loss'] = abs(o.loss.item() - want) / abs(want) / 5e-6
    errs['loss_part'] = abs(part[:nsl].sum() * inp.loss_scale - o.loss.item()) / abs(o.loss.item()) / 1e-12
    print(request.node.name, errs)
    record_errors(request.node.name, 0, errs)
    assert errs['dz'] <= 1 and errs['gw'] <= 1 and errs['gb'] <= 1 and errs.get('gwk', 0) <= 1
    assert errs['loss'] < 1 and errs['loss_part'] < 1
    assert int(o.ticket.item()) == 0
    assert np.all(part[nsl:] == FILL)            # one partial per slice, nothing past them
    # 5. guards, and every owned element of gW / gb written
    for buf, n in ((o.dzbuf, lo), (o.gWbuf, GUARD), (o.gbbuf, GUARD)):
        assert torch.all(buf[:n] == FILL) and torch.all(buf[-GUARD:] == FILL)
    assert not np.any(gW == FILL) and not np.any(gb == FILL)


CROSS = [pytest.param(Shape(1056, 256, 1000, 64, 1120, 5), 300, id='r1056-d256-V1000-stats2_dwo2'),
         pytest.param(Shape(512, 256, 1001, 128, 640, 5), 301, id='r512-d256-V1001-one_tile')]


@pytest.mark.parametrize('shape,seed', CROSS)
def test_dec_kl_deterministic(shape, seed):
    inp = _inputs(shape, 1, seed)
    assert _same(_run(inp), _run(inp))


@pytest.mark.parametrize('shape,seed', CROSS)
def test_dec_kl_no_state_left_in_ws(shape, seed):
    """A clip-live call, then a clip-free call on the same ws / ticket / loss partials: the second
    equals a clip-free call on a fresh zeroed ws (no stale fix flag, no stale delta partials)."""
    st = State(shape)
    _run(_inputs(shape, 1, seed), state=st)
    free = _inputs(shape, 0, seed)
    assert _same(_run(free, state=st), _run(free))


@pytest.mark.parametrize('shape,seed', CROSS)
def test_dec_kl_sharded_equals_unsharded(shape, seed):
    """Rows mt_lo .. of M~ resident with the shifted pointers = the whole M~ with mt_lo = 0."""
    inp = _inputs(shape, 1, seed)
    assert shape.mt_lo == 5 and int(inp.reg_idx[inp.reg_idx >= 0].min()) >= 5
    assert _same(_run(inp), _run(inp, mt_lo=0))


@pytest.mark.parametrize('shape,seed', CROSS)
def test_dec_kl_without_loss_out(shape, seed):
    """loss_out = NULL with ticket = NULL: every other output is the same."""
    inp = _inputs(shape, 1, seed)
    a, b = _run(inp), _run(inp, with_loss=False)
    assert _same(a, b, loss=False)
    assert b.loss.item() == FILL and int(b.ticket.item()) == 0


@pytest.mark.parametrize('V', [1, 7, 1001, 4096])
def test_kl_tsum(request, V):
    """cc_kl_tsum against fp64 sum t and sum t ln t, t = clip(Mt, 1e-7, 1): fp32 sums of V terms."""
    n = 9
    rng = np.random.default_rng(400 + V)
    Mt = rng.random((n, V)) ** 8
    if V >= 7:
        Mt /= Mt.sum(1, keepdims=True)
    Mt[0, ::3] = 0.0          # zeros among the entries
    Mt[1, 0] = 1.0            # exactly 1: t ln t = 0
    Mt[2, V // 2] = 1.5       # above 1: clipped
    Mt[3] = 0.0               # an all-zero row
    Mt = Mt.astype(np.float32)
    Md = torch.from_numpy(Mt).cuda()
    ts = torch.full((n, 2), FILL, device='cuda')
    L.call('cc_kl_tsum', L.ptr(Md), n, V, L.ptr(ts), L.stream_ptr())
    torch.cuda.synchronize()
    t = np.clip(Mt.astype(np.float64), 1e-7, 1.0)
    tl = t * np.log(t)
    got = ts.double().cpu().numpy()
    bound = (V + 2) * 2.0 ** -24
    errs = {'s': _ratio(np.abs(got[:, 0] - t.sum(1)), bound * np.abs(t).sum(1)),
            'c': _ratio(np.abs(got[:, 1] - tl.sum(1)), bound * np.abs(tl).sum(1))}
    print(request.node.name, errs)
    record_errors(request.node.name, 0, errs)
    assert errs['s'] <= 1 and errs['c'] <= 1
    # n = 0: CC_OK, nothing written
    ts0 = torch.full((n, 2), FILL, device='cuda')
    L.call('cc_kl_tsum', L.ptr(Md), 0, V, L.ptr(ts0), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.all(ts0 == FILL)
