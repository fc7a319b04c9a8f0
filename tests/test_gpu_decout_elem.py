"""cc_dec_bce_dw / cc_dec_bce_dw_ld / cc_dec_bce_dw_img (decout.hip, the fused D1 output layer) against
fp64, per element, at the smallest shapes that reach every instantiation of dec_bce_dw_kernel the host
entry can launch and every edge of its slices (run on an MI355X).  That is 21 of the 27 template
instantiations: the generic kernel at all nine (d, B), the DMA and the DMA+IMG kernel (Wo given in
place, V % 8 == 0) at the six (d <= 256, B); at d = 512 the host entry never launches a DMA kernel.
Twelve rows cover the edges; three more (V = 104, 40, 200) were added because those left the DMA
kernels of (d, B) = (128, 128), (128, 256) and (256, 256) — one pass with all eight waves busy at
B = 256, no priority switching — unreached: their only V were odd.  A module-level assert now
requires a V % 8 == 0 row for every (d <= 256, B).

The reference, the two input regimes (mild; trained: bo ~ -6, 2 % targets, all-zero D3 rows, columns
with bo = 0 / +-30 / +-100), the operand layouts and the derivation of every bound are in
tests/decout_ref.py, held to torch-CPU autograd and to six single-fault mutations by
tests/test_decout_ref_host.py.  In short (u = 2^-24, UB = 2^-8, scale = 1 / (B V)):
  eps_z = (d + 4) u (|D3| |Wo| + |bo|);  e = |dz| (eps_z + (|z| log2 e + 8) 2u);  tiny = 2^-126 scale
  dz    |dZ - dz| <= UB (|dz| + e) + e + tiny;  |dz| <= tiny: |dZ| <= tiny (dz_tiny);  else the signs agree
  gwk   |gW - D3^T dZ_kernel| <= (B + 2) u |D3|^T |dZ_kernel|
  gw    |gW - D3^T dz| <= |D3|^T dzb + (B + 2) u |D3|^T (|dz| + dzb)
  gb    |gb - colsum dz| <= (B + 2) u colsum |dz| + colsum (e + tiny)
  loss  per slice partial and for the total: sum (eps_z + 6u + 2^-126) + (16 NJ npass + 8) u sum terms
Every call uses the trainer's convention unless its form says otherwise: cc_dec_bce_dw_ld / _img, Wo
[d][V] read in place, the packed D3p / D3tp images of an ldt-row buffer whose rows B .. ldt hold 100.0,
dZ at the padded pitch ldz > V, loss_scale = 1 / (B V), a ticket word.  dZ, gW, gb and the loss partials
are prefilled with 7.0 and carry 64 guard elements on either side.  Per (row, regime) every operand form
the host entry can pick is run (FORMS) and all must agree bit for bit, guards and pad columns included;
the trainer's form is then compared with fp64.  Where V is a multiple of 64 (V = 768) the padded pitch
is one 64-column step wider than the trainer's, to keep pad columns to watch; the trainer's own call
there, _ld / _img at ldz = ceil64(V) = V with ldt = 2B, runs as two more forms (ld64, img64).

Observed error / bound per check, every row in both regimes (MI355X; the same values go to
$CCREC_PARITY_LOG through gpu_helpers.record_errors).  The forms of a row are bit-identical, so one
line stands for every kernel that ran on the row: g = generic alone; g, dma, img = generic, DMA and
DMA+IMG.  part_rel is loss_part_rel:
  B   d   V    kernels      regime   dz       gwk      gw       gb       loss_part loss     loss_rel part_rel
  128 128 1    g            mild     0.95     0.012    0.24     0.00044  6.6e-05  6.6e-05  4e-09    4e-09
  128 128 1    g            trained  0.94     0.0021   0.14     2.4e-05  0.00099  0.00099  4.3e-08  4.3e-08
  128 128 33   g            mild     0.98     0.016    0.28     0.0017   0.00079  0.00079  3.6e-08  3.6e-08
  128 128 33   g            trained  0.98     0.042    0.48     0.0015   4.6e-05  4.6e-05  2.4e-08  2.4e-08
  256 128 97   g            mild     0.98     0.014    0.21     0.0028   0.00026  0.00026  1.3e-08  1.3e-08
  256 128 97   g            trained  0.98     0.026    0.68     0.0015   9.2e-06  9.1e-06  6.5e-09  6.6e-09
  512 128 200  g, dma, img  mild     0.99     0.011    0.13     0.0023   0.00066  0.00049  2.4e-08  2.9e-08
  512 128 200  g, dma, img  trained  0.99     0.018    0.69     0.0016   2e-05    6.1e-06  4.4e-09  1.3e-08
  128 256 96   g, dma, img  mild     0.96     0.022    0.26     0.00095  0.00011  0.00011  1.4e-08  1.4e-08
  128 256 96   g, dma, img  trained  0.94     0.043    0.69     0.0013   1.3e-05  1.3e-05  1.6e-08  1.6e-08
  256 256 1001 g            mild     0.97     0.017    0.22     0.0016   0.00034  0.00013  1.6e-08  3.9e-08
  256 256 1001 g            trained  0.96     0.039    0.89     0.0011   1.6e-05  4.7e-06  6.9e-09  2.4e-08
  512 256 1000 g, dma, img  mild     0.98     0.012    0.16     0.0013   0.00025  0.00013  1.6e-08  3e-08
  512 256 1000 g, dma, img  trained  0.97     0.02     0.81     0.00096  2.1e-05  1.9e-06  2.9e-09  3e-08
  512 256 768  g, dma, img  mild     0.97     0.014    0.16     0.0014   0.00034  0.00016  2e-08    4.2e-08
  512 256 768  g, dma, img  trained  0.96     0.022    0.67     0.00084  1.9e-05  3.3e-06  4.9e-09  2.7e-08
  512 256 1001 g            mild     0.97     0.012    0.18     0.0014   0.00034  0.00018  2.2e-08  4.2e-08
  512 256 1001 g            trained  0.96     0.024    0.83     0.00081  1.4e-05  5.4e-06  8e-09    2e-08
  128 512 65   g            mild     0.94     0.022    0.26     0.0004   9.5e-06  9.4e-06  3.1e-09  3.1e-09
  128 512 65   g            trained  0.89     0.039    0.44     0.00045  3.8e-06  2.6e-06  6.7e-09  2.9e-08
  256 512 709  g            mild     0.94     0.021    0.22     0.0005   0.00015  6.8e-05  2.3e-08  5.1e-08
  256 512 709  g            trained  0.94     0.039    0.59     0.00047  9e-06    1.2e-06  4e-09    3e-08
  512 512 712  g            mild     0.94     0.013    0.17     0.0004   0.00014  6.5e-05  2.2e-08  4.7e-08
  512 512 712  g            trained  0.92     0.024    0.53     0.00038  1.1e-05  5.5e-07  1.9e-09  4.3e-08
  128 128 104  g, dma, img  mild     0.98     0.02     0.27     0.0026   0.00084  8.3e-05  3.9e-09  3.7e-08
  128 128 104  g, dma, img  trained  0.97     0.043    0.79     0.0035   2.4e-05  1.9e-05  1.1e-08  1.7e-08
  256 128 40   g, dma, img  mild     0.98     0.012    0.19     0.0019   0.00023  0.00023  1.1e-08  1.1e-08
  256 128 40   g, dma, img  trained  0.97     0.026    0.56     0.00098  2.2e-05  2.2e-05  1.7e-08  1.7e-08
  256 256 200  g, dma, img  mild     0.97     0.016    0.2      0.0012   0.00024  5.4e-05  6.6e-09  2.7e-08
  256 256 200  g, dma, img  trained  0.95     0.034    0.71     0.0008   3.6e-05  7.3e-06  1.1e-08  4.7e-08
dz_sign was 0 and loss_vs_partials (|sum of the partials x loss_scale - loss_out|, in units of 1e-14
relative) was 0 in every case.  A ratio above 1 is a finding about the kernel.
Near 1, as they should be: dz (half a bf16 ulp is the bound's own main term, and some element of
B V always sits at the edge of its rounding interval) and, in the trained regime, gw (the same
roundings pushed through |D3|^T: at 2 % targets almost every dz of a column has one sign, so they
hardly cancel).  dz_tiny is 0: where the reference dz is below tiny the kernel stores a zero.  With
slack: gwk (a worst-case bound of an error that grows like sqrt(B)), gb and above all the loss
(worst-case bounds — eps_z = (d + 4) u of the magnitude sum and 6 u per element, all one way — of
rounding errors that largely cancel over B and B NB terms; in the trained regime eps_z alone is
several per cent of a term of 0.0025, and the bound ~1e-3 of a slice's sum);
tests/test_decout_ref_host.py shows that each still fails on the single fault it exists for (a
16-row step dropped from dWo, a row dropped from dbo, a slice partial credited to another slice).
loss_rel and loss_part_rel are the plain relative errors of the total loss and of the worst slice
partial: <= 5.1e-8 in both regimes (mean loss 0.59 .. 0.78 mild, 0.13 .. 0.75 trained; the trained
slices past the first hold nothing but logits near -6), so the 1e-5 that
test_gpu_kernels.py::test_dec_bce_dw_matches_unfused claims — there checked at |z| ~ 1 - 3 only —
holds at trained logits too, with two orders of magnitude to spare; it is asserted here for the
total in both regimes, beside the derived bound.

Four one-line faults in a scratch build of decout.hip, each run against the first twelve rows of
this file on the MI355X (the three later rows are DMA rows with ldt = 2B like the V = 200 one):
the `gc2 < V` guard of the dWo stores removed (19 and 20 of the 24 elementwise cases fail in two
runs — the stray stores race with the owners' — on gwk / gw, or because the forms differ), the
`min(.., V - 1)` clamps of the Wo staging one column early (22 fail, all but
V = 1: dz of the last column, or — where the trainer's form is the DMA kernel, which has no clamp —
the forms differ), `ldt` replaced by B in phase 2 (all 18 cases with ldt > B fail: gwk, gw), `LZ`
replaced by V in the dZ store offset (all 24 fail: dz, and the pad columns are written).
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from tests import decout_ref as DR
from tests.gpu_helpers import record_errors

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 7.0
EXTRA = 8          # loss partial entries past cc_dec_bce_dw_blocks(V)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    L.lib()


# entry: 'ld' | 'img' | 'plain' (cc_dec_bce_dw: ldt = B, ldz = V) | 'ld64' / 'img64' (_ld / _img with ldt = 2B at
# the trainer's own pitch ceil64(V); run where that differs from decout_ref.ldz_of(V), i.e. where it has no pad
# columns: V % 64 == 0);  wot: Wo^T [V][d] given instead of Wo;  packed: the D3p / D3tp images given
Form = namedtuple('Form', 'entry wot packed')
TRAINER = Form('ld', False, True)
FORMS = [TRAINER, Form('ld', True, True), Form('ld', False, False), Form('ld', True, False),
         Form('img', False, True), Form('img', False, False), Form('img', True, True), Form('plain', False, True),
         Form('plain', True, False), Form('ld64', False, True), Form('img64', False, True)]


def variant(case, form):
    """The kernel the host entry picks."""
    if form.wot or case.V % 8 or case.d > 256:
        return 'generic'
    return 'dma+img' if form.entry.startswith('img') else 'dma'


def _dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16).cuda()


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


@functools.lru_cache(maxsize=2)
def _case(case, regime):
    """Inputs, reference (computed once, shared, never written) and the host operand images."""
    inp = DR.case_inputs(case, regime)
    return inp, DR.reference(inp), DR.operand_images(inp), DR.operand_images(inp, ldt=case.B)


class State:
    """What a caller keeps between calls: the loss partials and the ticket."""

    def __init__(self, case, ticket=0):
        self.nblk = int(L.lib().cc_dec_bce_dw_blocks(case.V))
        self.part = torch.full((GUARD + self.nblk + EXTRA + GUARD,), FILL, device='cuda', dtype=torch.float64)
        self.ticket = torch.full((3,), ticket, device='cuda', dtype=torch.int32)


Out = namedtuple('Out', 'dzbuf gWbuf gbbuf loss part ticket ldz')


def _run(inp, form=TRAINER, state=None, with_loss=True, with_ticket=True):
    """One call.  dZ (B * ldz elements), gW, gb and the loss partials are prefilled with FILL and carry
    GUARD elements on either side of what the kernel owns; loss is prefilled; the ticket is caller state."""
    case = inp.case
    B, d, V, ldt = case
    _, _, im_ldt, im_b = _case(case, inp.regime)
    plain = form.entry == 'plain'
    im, ldt, ldz = (im_b, B, V) if plain else (im_ldt, ldt, DR.ldz_of(V))
    if form.entry.endswith('64'):      # the trainer with the regulariser on: ldt = 2B, ldz = ceil64(V)
        ldt, ldz = 2 * B, DR.ceil64(V)
        im = DR.operand_images(inp, ldt=ldt)
    state = state or State(case)
    D3, D3t = _dev_bf16(im.D3), _dev_bf16(im.D3t)
    D3p, D3tp = (_dev_bf16(im.D3p), _dev_bf16(im.D3tp)) if form.packed else (None, None)
    W = _dev_bf16(im.WoT if form.wot else im.Wo)
    bo = torch.from_numpy(inp.bo.astype(np.float32)).cuda()
    yb = _dev_u32(inp.ybits)
    dzbuf = torch.full((GUARD + B * ldz + GUARD,), FILL, device='cuda', dtype=torch.bfloat16)
    gWbuf = torch.full((GUARD + d * V + GUARD,), FILL, device='cuda')
    gbbuf = torch.full((GUARD + V + GUARD,), FILL, device='cuda')
    loss = torch.full((1,), FILL, device='cuda', dtype=torch.float64)
    head = (L.ptr(D3), L.ptr(D3t), ldt, L.ptr(D3p), L.ptr(D3tp), L.ptr(W) if form.wot else None,
            None if form.wot else L.ptr(W), L.ptr(bo), B, d, V, L.ptr(yb))
    tail = (gWbuf.data_ptr() + 4 * GUARD, gbbuf.data_ptr() + 4 * GUARD, state.part.data_ptr() + 8 * GUARD,
            L.ptr(loss) if with_loss else None, inp.scale, state.ticket.data_ptr() + 4 if with_ticket else None,
            L.stream_ptr())
    dz = dzbuf.data_ptr() + 2 * GUARD
    if plain:
        L.call('cc_dec_bce_dw', *head, dz, *tail)
    elif form.entry.startswith('img'):
        yi = _dev_u32(DR.y_img_of(inp.ybits))
        assert yi.data_ptr() % 128 == 0
        L.call('cc_dec_bce_dw_img', *head, L.ptr(yi), dz, ldz, *tail)
    else:
        L.call('cc_dec_bce_dw_ld', *head, dz, ldz, *tail)
    torch.cuda.synchronize()
    return Out(dzbuf.cpu(), gWbuf.cpu(), gbbuf.cpu(), loss.cpu(), state.part.cpu(), state.ticket.cpu(), ldz)


def _dz_rows(o, case):
    """The dZ buffer's B rows of ldz elements, as int16 bit patterns."""
    return o.dzbuf[GUARD:GUARD + case.B * o.ldz].view(torch.int16).view(case.B, o.ldz)


def _same(a, b, case, loss=True):
    """Bit-identical outputs: whole buffers (guards and pad columns included) at equal pitch, the
    owned dZ columns otherwise."""
    if a.ldz == b.ldz:
        ok = torch.equal(a.dzbuf.view(torch.int16), b.dzbuf.view(torch.int16))
    else:
        ok = torch.equal(_dz_rows(a, case)[:, :case.V], _dz_rows(b, case)[:, :case.V])
    ok = ok and torch.equal(a.gWbuf.view(torch.int32), b.gWbuf.view(torch.int32))
    ok = ok and torch.equal(a.gbbuf.view(torch.int32), b.gbbuf.view(torch.int32)) and torch.equal(a.part, b.part)
    return ok and (not loss or torch.equal(a.loss, b.loss))


def _untouched(o, case):
    """Guards, pad columns, the loss partials past the grid, the ticket's neighbours: all still FILL
    (or the ticket's initial value), byte for byte; every owned element written."""
    B, d, V, ldt = case
    fill16 = torch.tensor([FILL], dtype=torch.bfloat16).view(torch.int16).item()
    nsl = DR.n_slices(d, V)
    for buf in (o.dzbuf, o.gWbuf, o.gbbuf, o.part):
        assert torch.all(buf[:GUARD] == FILL) and torch.all(buf[-GUARD:] == FILL)
    rows = _dz_rows(o, case)
    assert torch.all(rows[:, V:] == fill16), 'a dZ store in the pad columns'
    assert not torch.any(rows[:, :V] == fill16), 'an owned dZ element not written'
    assert not torch.any(o.gWbuf[GUARD:-GUARD] == FILL) and not torch.any(o.gbbuf[GUARD:-GUARD] == FILL)
    assert torch.all(o.part[GUARD + nsl:] == FILL), 'a loss partial past the grid'
    assert not torch.any(o.part[GUARD:GUARD + nsl] == FILL)


# what each row reaches (B, d, V, ldt in decout_ref.CASES, the same order)
REACHES = ['one_column_one_word_one_block_waves_4_7_idle', 'odd_V_two_words_one_partial_slice',
           'second_slice_of_one_column_one_pass', 'V%8_dma_img_two_passes_8col_last_slice', 'exactly_one_slice_dma',
           'odd_V_11_blocks_remap_remainder_element_loads', 'split2_dma_img_11_blocks_40col_tail',
           'split2_exactly_8_slices_remap_remainder_0', 'split2_generic_odd_V', '64col_slices_one_column_tail_A_ring',
           'd512_odd_V_12_blocks', 'd512_V%8_vector_Wo_loads_element_loads_in_8col_last_block',
           'dma_img_B128_two_blocks_8col_last_slice', 'dma_img_B256_d128_one_block_two_words',
           'dma_img_B256_d256_three_blocks']
assert len(REACHES) == len(DR.CASES)
# every instantiation the host entry can launch: the generic kernel at all nine (d, B); the DMA and DMA+IMG
# kernels (never launched at d = 512) at the six (d <= 256, B), which need a row with V % 8 == 0
assert {(c.d, c.B) for c in DR.CASES} == {(d, B) for d in (128, 256, 512) for B in (128, 256, 512)}
assert {(c.d, c.B) for c in DR.CASES if c.V % 8 == 0 and c.d <= 256} == {(d, B) for d in (128, 256)
                                                                         for B in (128, 256, 512)}
PARAMS = [pytest.param(c, r, id=f'B{c.B}-d{c.d}-V{c.V}-ldt{c.ldt}-{name}-{r}')
          for c, name in zip(DR.CASES, REACHES) for r in DR.REGIMES]


@pytest.mark.parametrize('case,regime', PARAMS)
def test_dec_bce_elementwise(request, case, regime):
    """Every operand form of one row bit-identical; the trainer's form against the fp64 reference,
    every output element (module docstring: the bounds)."""
    B, d, V, ldt = case
    inp, ref, _, _ = _case(case, regime)
    assert ldt >= B and DR.ldz_of(V) > V and DR.ldz_of(V) % 64 == 0
    o = _run(inp)
    # 1. against fp64 (every figure printed and recorded before anything is asserted)
    nsl = DR.n_slices(d, V)
    dZ = o.dzbuf[GUARD:GUARD + B * o.ldz].view(B, o.ldz)[:, :V].double().numpy()
    gW = o.gWbuf[GUARD:GUARD + d * V].view(d, V).double().numpy()
    gb = o.gbbuf[GUARD:GUARD + V].double().numpy()
    part = o.part[GUARD:GUARD + nsl].numpy()
    errs = DR.compare(inp, ref, dZ, gW, gb, part, o.loss.item())
    errs['loss_vs_partials'] = abs(part.sum() * inp.scale - o.loss.item()) / abs(o.loss.item()) / 1e-14
    variants = sorted({variant(case, f) for f in FORMS})
    assert variants == (['dma', 'dma+img', 'generic'] if V % 8 == 0 and d <= 256 else ['generic'])
    print(request.node.name, '+'.join(variants), errs)
    record_errors(request.node.name, 0, errs)
    assert DR.passes(errs), errs
    assert errs['loss_vs_partials'] <= 1
    assert errs['loss_rel'] <= 1e-5       # the claim of test_dec_bce_dw_matches_unfused, in both regimes
    # 2. untouched memory, written memory, the ticket
    _untouched(o, case)
    assert o.ticket.tolist() == [0, 0, 0]
    # 3. every other form: the same bits
    for form in FORMS[1:]:
        if form.entry.endswith('64') and DR.ceil64(V) == DR.ldz_of(V):
            continue       # the trainer's own pitch is the one every 'ld' / 'img' form has used
        f = _run(inp, form)
        assert _same(o, f, case), f'{form} ({variant(case, form)}) differs from the trainer\'s form'
        assert f.ticket.tolist() == [0, 0, 0]
        if form.entry != 'ld' and form.entry != 'img':   # no pad columns: the guards sit right at the end of a row
            _untouched(f, case)


CROSS = [pytest.param(DR.CASES[6], id='B512-d256-V1000-split2'), pytest.param(DR.CASES[10], id='B256-d512-V709-ring')]


@pytest.mark.parametrize('case', CROSS)
def test_dec_bce_deterministic(case):
    inp = _case(case, 'trained')[0]
    for form in (TRAINER, Form('img', False, True)):
        assert _same(_run(inp, form), _run(inp, form), case)


@pytest.mark.parametrize('case', CROSS)
def test_dec_bce_no_state_left(case):
    """A trained-regime call, then a mild one on the same ticket and loss partials: the second equals
    a mild call on fresh state."""
    st = State(case)
    first = _run(_case(case, 'trained')[0], state=st)
    assert first.ticket.tolist() == [0, 0, 0]
    mild = _case(case, 'mild')[0]
    again, fresh = _run(mild, state=st), _run(mild)
    assert _same(again, fresh, case) and again.ticket.tolist() == [0, 0, 0]
    assert not torch.equal(first.part, again.part)


@pytest.mark.parametrize('with_ticket', [True, False], ids=['ticket', 'no_ticket'])
@pytest.mark.parametrize('case', CROSS)
def test_dec_bce_without_loss_out(case, with_ticket):
    """loss_out = NULL: every other output is the same, loss keeps its prefill, the ticket word is
    not touched (it holds 3 before and after)."""
    inp = _case(case, 'trained')[0]
    a = _run(inp)
    b = _run(inp, state=State(case, ticket=3), with_loss=False, with_ticket=with_ticket)
    assert _same(a, b, case, loss=False)
    assert b.loss.item() == FILL and b.ticket.tolist() == [3, 3, 3]
    _untouched(b, case)
