"""tests/decout_ref.py (the fp64 reference, inputs, layouts and bounds of tests/test_gpu_decout_elem.py)
on the host: the reference against torch-CPU autograd in float64 (so it is not its own judge), the
layout builders against the index formulas of include/ccrec.h, the conditions on the inputs that the
comparison relies on, and the bounds themselves on a simulated kernel — fp32 logits in numpy's order
and the kernel's fp32 epilogue formula, which they must pass in both regimes, and six single-fault
mutations, each of which must push its own ratio above 1."""
import functools

import numpy as np
import pytest
import torch

from tests import decout_ref as DR
from tests import tower_ref as TR
from tests.gpu_helpers import rel_err

F = np.float32


@functools.lru_cache(maxsize=2)
def _case(case, regime):
    inp = DR.case_inputs(case, regime)
    return inp, DR.reference(inp)


@pytest.mark.parametrize('regime', DR.REGIMES)
@pytest.mark.parametrize('case', [DR.Case(128, 128, 33, 256), DR.Case(256, 256, 1001, 512), DR.Case(128, 512, 65, 256)],
                         ids=lambda c: f'B{c.B}-d{c.d}-V{c.V}')
def test_reference_matches_torch_autograd(case, regime):
    inp, ref = _case(case, regime)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    W, b = t(inp.Wo), t(inp.bo)
    z = torch.tensor(inp.D3) @ W + b
    z.retain_grad()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z, torch.tensor(inp.y.astype(np.float64)))
    loss.backward()
    tol = 1e-12
    assert abs(ref.loss - loss.item()) <= tol * abs(loss.item())
    assert rel_err(ref.dz, z.grad.numpy()) < tol
    assert np.max(np.abs(ref.dz - z.grad.numpy())) <= tol * inp.scale      # per element, not only in the norm
    assert rel_err(ref.gW, W.grad.numpy()) < tol
    assert rel_err(ref.gb, b.grad.numpy()) < tol
    assert abs(ref.slice_sums.sum() * inp.scale - ref.loss) <= tol * ref.loss
    NB = DR.nb_of(case.d)
    assert len(ref.slice_sums) == DR.n_slices(case.d, case.V)
    assert ref.slice_sums[-1] == ref.terms[:, (len(ref.slice_sums) - 1) * NB:].sum()


def test_layout_helpers():
    case = DR.Case(128, 128, 33, 256)
    B, d, V, ldt = case
    inp = DR.case_inputs(case, 'trained')
    # an operand whose every element names itself
    X = (np.arange(B * d, dtype=np.int64).reshape(B, d) % 251 + 1).astype(np.float64)
    im = DR.operand_images(inp._replace(D3=X))
    Xb, loud = TR.bits(X), TR.bits(F(DR.LOUD))
    assert loud == 0x42C8 and TR.from_bits(loud) == 100.0
    assert im.D3.shape == (ldt, d) and np.array_equal(im.D3[:B], Xb) and np.all(im.D3[B:] == loud)
    assert im.D3t.shape == (d, ldt) and np.array_equal(im.D3t[:, :B], Xb.T) and np.all(im.D3t[:, B:] == loud)
    # act6p: fragment (row block t, j), lane l: row 32t + (l & 31), columns 16j + 8(l >> 5) .. + 8
    P = im.D3p.reshape(ldt // 32, d // 16, 64, 8)
    for t, j, l in ((0, 0, 0), (2, 3, 37), (1, 7, 63), (3, 0, 31)):
        c = 16 * j + 8 * (l >> 5)
        assert np.array_equal(P[t, j, l], Xb[32 * t + (l & 31), c:c + 8])
    assert np.all(P[B // 32:] == loud)
    assert np.array_equal(TR.unpack_rows(im.D3p, ldt, d), im.D3)
    # act6tp: fragment (feature block t, j), lane l: feature 32t + (l & 31), batch rows 16j + 8(l >> 5) .. + 8
    P = im.D3tp.reshape(d // 32, ldt // 16, 64, 8)
    for t, j, l in ((0, 0, 0), (1, 5, 37), (3, 2, 63), (2, 7, 31)):
        r = 16 * j + 8 * (l >> 5)
        assert np.array_equal(P[t, j, l], Xb[r:r + 8, 32 * t + (l & 31)])
    assert np.all(P[:, B // 16:] == loud)
    assert np.array_equal(TR.unpack_t(im.D3tp, d, ldt), im.D3)
    # the expressions of test_gpu_kernels.py::test_dec_bce_dw_matches_unfused, on the ldt-row buffer
    D3 = torch.from_numpy(im.D3.view(np.int16))
    u16 = lambda t: t.reshape(-1).numpy().view(np.uint16)
    assert np.array_equal(u16(D3.view(ldt // 32, 32, d // 16, 2, 8).permute(0, 2, 3, 1, 4)), im.D3p)
    D3t = D3.t().contiguous()
    assert np.array_equal(u16(D3t.view(d // 32, 32, ldt // 16, 2, 8).permute(0, 2, 3, 1, 4)), im.D3tp)
    assert np.array_equal(im.WoT, im.Wo.T) and np.array_equal(TR.from_bits(im.Wo), inp.Wo)
    # y_bits: bit l of word w of row b is column 32 w + l; the last word's bits past V are random
    yb = inp.ybits
    VW = (V + 31) // 32
    assert yb.shape == (B, VW) and yb.dtype == np.uint32
    for b, c in ((0, 0), (5, 31), (77, 32), (127, 17)):
        assert (int(yb[b, c >> 5]) >> (c & 31)) & 1 == int(inp.y[b, c])
    assert np.array_equal(DR.unpack_y_bits(yb, V), inp.y)
    past = yb[:, -1] >> np.uint32(V & 31)
    assert 0.3 < np.mean([(int(w) >> k) & 1 for w in past for k in range(32 - (V & 31))]) < 0.7
    assert np.all(DR.y_bits_of(inp.y)[:, -1] >> np.uint32(V & 31) == 0)
    assert np.array_equal(DR.y_bits_of(inp.y) & np.uint32(1), yb & np.uint32(1))
    # y_img: [VW][B], dword 2r + h of a 32-row block = the block's row (r & 3) + 8 (r >> 2) + 4h
    img = DR.y_img_of(yb)
    assert img.shape == (VW, B)
    for w, blk, r, h in ((0, 0, 0, 0), (1, 3, 15, 1), (0, 2, 6, 1), (1, 1, 9, 0)):
        assert img[w, 32 * blk + 2 * r + h] == yb[32 * blk + (r & 3) + 8 * (r >> 2) + 4 * h, w]
    pos = torch.arange(32)
    row = 8 * (pos >> 3) + 4 * (pos & 1) + ((pos >> 1) & 3)
    ybt = torch.from_numpy(yb.view(np.int32))
    want = ybt[(torch.arange(B // 32)[:, None] * 32 + row[None, :]).reshape(-1)].t().contiguous()
    assert np.array_equal(want.numpy().view(np.uint32), img)
    assert np.array_equal(np.sort(img, axis=1), np.sort(yb.T, axis=1))      # a permutation of the rows


@pytest.mark.parametrize('case', DR.CASES, ids=lambda c: f'B{c.B}-d{c.d}-V{c.V}')
def test_input_conditions(case):
    """What the GPU comparison relies on, for every case it runs."""
    B, d, V, ldt = case
    for regime in DR.REGIMES:
        inp, ref = _case(case, regime)
        assert DR.input_conditions(inp, ref) == [], (regime, DR.input_conditions(inp, ref))
        assert 0.35 < np.mean(inp.D3 == 0) < 0.65 and inp.D3.min() == 0       # a ReLU output
        assert np.array_equal(TR.round_bf16(inp.D3), inp.D3) and np.array_equal(TR.round_bf16(inp.Wo), inp.Wo)
        assert np.array_equal(inp.bo.astype(F).astype(np.float64), inp.bo)
        assert ldt >= B and ldt % 32 == 0 and V < DR.ldz_of(V) <= V + 64 and DR.ldz_of(V) % 64 == 0
    inp, ref = _case(case, 'mild')
    if V > 1:
        assert 0.5 < ref.z.std() < 1.2
    for c0 in range(0, V, 32):     # a tile whose targets are all alike checks no mask
        t = inp.y[:, c0:c0 + 32]
        assert t.any() and not t.all(), c0
    inp, ref = _case(case, 'trained')
    zr = list(inp.zero_rows)
    assert len(set(zr)) == 4 and np.all(inp.D3[zr] == 0)
    assert np.array_equal(ref.z[zr], np.broadcast_to(inp.bo, (4, V)))          # z == bo exactly
    classes = {k for _, k in inp.planted}
    assert classes == (set(range(len(DR.EDGES))) if V >= 10 else set(range(len(inp.planted))))
    for c, k in inp.planted:
        assert inp.bo[c] == DR.EDGES[k] and np.all(ref.z[zr, c] == DR.EDGES[k])
        assert set(inp.y[zr, c]) == {False, True} and set(inp.y[:, c]) == {False, True}
    if V >= 10:
        assert any(np.signbit(inp.bo[c]) for c, k in inp.planted if k == 0)    # a -0.0 bias
        assert V - 1 not in [c for c, _ in inp.planted]
        plain = np.setdiff1d(np.arange(V), [c for c, _ in inp.planted])
        assert abs(inp.bo[plain].mean() + 6) < 1 and 0.005 < inp.y[:, plain].mean() < 0.04
    # saturation is reached: a underflows in fp32 at +-100, and sigmoid is 0 or 1 to fp32 at +-30
    if V >= 10:
        assert np.any(np.abs(ref.z) * DR.LOG2E > 126) and np.any(np.abs(ref.dz) <= DR.tiny_of(inp))


# ------------------------------------------------------------------ a simulated kernel
def simulate(inp, y=None, Wo=None, trunc=False):
    """A kernel that is right: z in fp32 (numpy's own order), the epilogue in fp32 by the kernel's
    formula — a = exp2(-|z log2e|), 1 / (1 + a), the product of a lane's sixteen 1 + a (rows
    (r & 3) + 8 (r >> 2) + 4h of a 32-row block) before one log — dZ rounded once to bf16, dWo in fp32
    from the rounded dZ, dbo from the unrounded dz.  -> dZ, gW, gb, slice partials, loss (fp64 values)."""
    B, d, V, ldt = inp.case
    y = inp.y if y is None else y
    Wo = inp.Wo if Wo is None else Wo
    z = inp.D3.astype(F) @ Wo.astype(F) + inp.bo.astype(F)
    a = np.exp2(-np.abs(z * F(DR.LOG2E)))
    opa = F(1) + a
    rp = F(1) / opa
    sn = (z < 0) != y
    scale = F(1) / (F(B) * F(V))
    mag = np.where(sn, a * rp, rp) * scale
    dz = np.where(y, -mag, mag)
    assert z.dtype == F and dz.dtype == F
    if trunc:     # toward zero instead of to nearest even
        dZ = ((dz.view(np.uint32) >> np.uint32(16)) << np.uint32(16)).view(F).astype(np.float64)
    else:
        dZ = TR.round_bf16(dz)
    rl = np.where(sn, F(0), np.abs(z))
    prod = opa.reshape(B // 32, 4, 2, 4, V).prod(axis=(1, 3), dtype=F)      # row = 32 blk + 8 g + 4 h + i
    lg = np.log2(prod)
    NB = DR.nb_of(d)
    part = np.array([rl[:, n:n + NB].sum(dtype=F) + lg[..., n:n + NB].sum(dtype=F) * F(np.log(2.0))
                     for n in range(0, V, NB)], np.float64)
    gW = (inp.D3.astype(F).T @ dZ.astype(F)).astype(np.float64)
    gb = dz.sum(0, dtype=F).astype(np.float64)
    return dZ, gW, gb, part, part.sum() * inp.scale


SIM = [DR.Case(256, 128, 97, 512), DR.Case(512, 256, 1000, 1024), DR.Case(128, 512, 65, 256),
       DR.Case(256, 512, 709, 512)]


@pytest.mark.parametrize('regime', DR.REGIMES)
@pytest.mark.parametrize('case', SIM, ids=lambda c: f'B{c.B}-d{c.d}-V{c.V}')
def test_bounds_pass_a_right_kernel_and_fail_a_wrong_one(case, regime):
    B, d, V, ldt = case
    inp, ref = _case(case, regime)
    dZ, gW, gb, part, loss = simulate(inp)
    errs = DR.compare(inp, ref, dZ, gW, gb, part, loss)
    print(case, regime, errs)
    assert DR.passes(errs), errs
    assert errs['loss_rel'] < 1e-5
    bad = lambda **kw: DR.compare(inp, ref, **{**dict(dZ=dZ, gW=gW, gb=gb, part=part, loss=loss), **kw})
    # 1. dz truncated toward zero instead of rounded to nearest even
    assert bad(dZ=simulate(inp, trunc=True)[0])['dz'] > 1
    # 2. one target bit flipped: an ordinary element, and one of each target value
    for want in (False, True):
        r, c = np.argwhere(inp.y == want)[11]
        y2 = inp.y.copy()
        y2[r, c] ^= True
        e2 = bad(dZ=simulate(inp, y=y2)[0])
        assert e2['dz'] > 1 and e2['dz_sign'] == 1
    # 3. the last live column computed from its neighbour's weights (the slice-edge clamp one column early)
    Wo2 = inp.Wo.copy()
    Wo2[:, V - 1] = Wo2[:, V - 2]
    assert bad(dZ=simulate(inp, Wo=Wo2)[0])['dz'] > 1
    # 4. one 16-row step dropped from one d tile of dWo
    keep = np.r_[0:B - 32, B - 16:B]
    gW2 = gW.copy()
    gW2[32:64] = (inp.D3[keep, 32:64].astype(F).T @ dZ[keep].astype(F)).astype(np.float64)
    e4 = bad(gW=gW2)
    assert e4['gwk'] > 1 and e4['gw'] > 1
    # 5. rows rl and rl + 4 of one 32-row block swapped in the masks
    blk = B // 32 - 1
    rl = next(r for r in (0, 1, 2, 3, 8, 9, 10, 11) if np.any(inp.y[32 * blk + r] != inp.y[32 * blk + r + 4]))
    y5 = inp.y.copy()
    y5[[32 * blk + rl, 32 * blk + rl + 4]] = y5[[32 * blk + rl + 4, 32 * blk + rl]]
    assert bad(dZ=simulate(inp, y=y5)[0])['dz'] > 1
    # 6. one slice's loss partial credited to another slice (the total is unchanged)
    part6 = part.copy()
    part6[[0, 1]] = part6[[1, 0]]
    e6 = bad(part=part6)
    assert e6['loss_part'] > 1 and e6['loss'] <= 1
    # ... and a partial lost altogether shows in the total
    assert bad(loss=(part.sum() - part[-1]) * inp.scale)['loss'] > 1
    # the bias gradient: one row's dz (the column's largest) left out of one column
    gb2 = gb.copy()
    gb2[V // 2] -= dZ[np.argmax(np.abs(dZ[:, V // 2])), V // 2]
    assert bad(gb=gb2)['gb'] > 1
