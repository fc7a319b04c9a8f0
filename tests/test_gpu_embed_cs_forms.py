"""GPU: the Adam and reg-by-index forms of the column-slice W1 gradient at kernel level, bit for
bit against the plain form (cc_embed_grad_cs, itself pinned to cc_embed_grad_mfma in
test_gpu_kernels.py): cc_embed_grad_cs_adam == cc_embed_grad_cs + cc_adam_dense over W1;
cc_embed_grad_cs_reg / cc_embed_grad_cs_adam_reg == the plain product over R + nreg bit rows;
cc_embed_grad_cs_reg by row chunk (card0) == one launch.  V = 777: 25 tiles, the bias row inside
the partial last one."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L

pytestmark = pytest.mark.gpu

V, D = 777, 128
ADAM = (1e-3, 0.9, 0.999, 1e-7)


def _bits(X):
    """[rows][V] bool -> the transposed bit matrix [V][ceil(rows / 32)] (int32 words)."""
    rows = X.shape[0]
    xt = np.zeros((V, (rows + 31) // 32), np.uint32)
    rr, cc = np.nonzero(X)
    np.bitwise_or.at(xt, (cc, rr // 32), (np.uint32(1) << (rr % 32).astype(np.uint32)))
    return torch.from_numpy(xt.view(np.int32)).cuda()


def _image(rows, packed, gen):
    """A dPre1 image of `rows` rows (pitch ceil64): packed transposed fragments or dPre1^T."""
    RP = (rows + 63) // 64 * 64
    gpad = torch.zeros(RP, D, device='cuda', dtype=torch.bfloat16)
    gpad[:rows] = (torch.randn(rows, D, device='cuda', generator=gen) * 0.1).to(torch.bfloat16)
    if packed:
        return gpad.view(RP // 16, 2, 8, D // 32, 32).permute(3, 0, 1, 4, 2).contiguous(), RP
    return gpad.t().contiguous(), RP


def _moments(gen):
    return (torch.randn(V * D, device='cuda', generator=gen) * 0.05,
            torch.randn(V * D, device='cuda', generator=gen) * 1e-3,
            torch.rand(V * D, device='cuda', generator=gen) * 1e-5)


def _tickets(R):
    return torch.zeros(int(L.lib().cc_embed_grad_cs_tickets(V, D, R)), device='cuda', dtype=torch.int32)


def _plain(img, packed, R, RP, xt):
    """cc_embed_grad_cs: (grad, bias_grad); the bit words consumed, the tickets left zero."""
    xt, tk = xt.clone(), _tickets(R)
    grad, bg = torch.full((V, D), 7.0, device='cuda'), torch.full((D,), 7.0, device='cuda')
    L.call('cc_embed_grad_cs', L.ptr(img), packed, V, D, R, RP, L.ptr(xt), L.ptr(grad), L.ptr(bg), L.ptr(tk),
           L.stream_ptr())
    torch.cuda.synchronize()
    assert int(xt.abs().sum().item()) == 0 and int(tk.abs().sum().item()) == 0
    return grad, bg


def _adam_dense(grad, pmv, state):
    """cc_adam_dense over W1's V * d elements: (p, m, v, shadow)."""
    p, m, v = (x.clone() for x in pmv)
    shadow = torch.zeros(V * D, device='cuda', dtype=torch.bfloat16)
    L.call('cc_adam_dense', L.ptr(p), L.ptr(m), L.ptr(v), L.ptr(grad), L.ptr(shadow), V * D, L.ptr(state), *ADAM,
           L.stream_ptr())
    torch.cuda.synchronize()
    return p, m, v, shadow


def _adam_form(img, packed, R, RP, xt, pmv, state, reg=()):
    """cc_embed_grad_cs_adam[_reg]: (p, m, v, shadow, bias_grad)."""
    xt, tk = xt.clone(), _tickets(R)
    p, m, v = (x.clone() for x in pmv)
    shadow = torch.zeros(V * D, device='cuda', dtype=torch.bfloat16)
    bg = torch.full((D,), 7.0, device='cuda')
    L.call('cc_embed_grad_cs_adam' + ('_reg' if reg else ''), L.ptr(img), packed, V, D, R, RP, L.ptr(xt), L.ptr(bg),
           L.ptr(tk), L.ptr(p), L.ptr(m), L.ptr(v), L.ptr(shadow), L.ptr(state), *ADAM, *reg, L.stream_ptr())
    torch.cuda.synchronize()
    assert int(xt.abs().sum().item()) == 0 and int(tk.abs().sum().item()) == 0   # consumed, tickets reset
    return p, m, v, shadow, bg


def _same(got, want, names):
    bad = [n for n, a, b in zip(names, got, want) if not torch.equal(a, b)]
    assert not bad, bad


# R = 96 / 512: the 16-word instance with scalar / 16-B bit loads; 544 / 1024: the 32-word one
@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('R', [96, 512, 544, 1024])
def test_adam_form_matches_plain_then_adam_dense(R, packed):
    gen = torch.Generator(device='cuda').manual_seed(R + packed)
    rng = np.random.default_rng(R + packed)
    img, RP = _image(R, packed, gen)
    xt = _bits(rng.random((R, V)) < 0.05)
    pmv = _moments(gen)
    state = torch.tensor([4, 0, 0, 0], device='cuda', dtype=torch.int64)
    grad, bg = _plain(img, packed, R, RP, xt)
    want = _adam_dense(grad, pmv, state) + (bg,)
    assert not torch.equal(want[0], pmv[0]) and not bool((bg == 7.0).any())
    _same(_adam_form(img, packed, R, RP, xt, pmv, state), want, 'p m v shadow bias_grad'.split())


def _reg_problem(R, nreg, packed):
    """R cube rows and nreg reg rows behind them in one dPre1 image: the bit matrix of all R + nreg
    rows (row R + i: the bit of card reg_idx[i], none for a padding row) and of the cube rows."""
    gen = torch.Generator(device='cuda').manual_seed(3 * R + packed)
    rng = np.random.default_rng(3 * R + packed)
    img, RP = _image(R + nreg, packed, gen)
    rid = rng.integers(0, V, nreg).astype(np.int32)
    rid[[1, 2, 3, 4, 5, 6, 8, 9]] = V - 1     # a popular card (the last one: the tile of the bias row)
    rid[::7] = -1                             # padding rows
    X = np.zeros((R + nreg, V), bool)
    X[:R] = rng.random((R, V)) < 0.05
    real = np.nonzero(rid >= 0)[0]
    X[R + real, rid[real]] = True
    return gen, img, RP, _bits(X), _bits(X[:R]), torch.from_numpy(rid).cuda()


@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('R', [96, 544])
def test_reg_forms_match_plain_over_all_rows(R, packed):
    nreg = 64
    gen, img, RP, xt_all, xt_cube, rid = _reg_problem(R, nreg, packed)
    pmv = _moments(gen)
    state = torch.tensor([4, 0, 0, 0], device='cuda', dtype=torch.int64)
    grad, bg = _plain(img, packed, R + nreg, RP, xt_all)
    assert not bool((grad == 7.0).any()) and not bool((bg == 7.0).any())
    reg = (L.ptr(rid), nreg, R // 16)
    xt, tk = xt_cube.clone(), _tickets(R)
    g2, b2 = torch.full((V, D), 7.0, device='cuda'), torch.full((D,), 7.0, device='cuda')
    L.call('cc_embed_grad_cs_reg', L.ptr(img), packed, V, D, R, RP, L.ptr(xt), L.ptr(g2), L.ptr(b2), L.ptr(tk), *reg,
           0, L.stream_ptr())
    torch.cuda.synchronize()
    assert int(xt.abs().sum().item()) == 0 and int(tk.abs().sum().item()) == 0
    _same((g2, b2), (grad, bg), ('grad', 'bias_grad'))
    want = _adam_dense(grad, pmv, state) + (bg,)
    _same(_adam_form(img, packed, R, RP, xt_cube, pmv, state, reg), want, 'p m v shadow bias_grad'.split())


@pytest.mark.parametrize('packed', [0, 1])
def test_reg_form_by_row_chunk_matches_one_launch(packed):
    """The data-parallel trainer's use: W1 rows [0, 384) and [384, 777) one launch each, card0 the
    chunk's first row, the bias row with the last chunk."""
    R, nreg = 96, 64
    _, img, RP, _, xt_cube, rid = _reg_problem(R, nreg, packed)
    reg = (L.ptr(rid), nreg, R // 16)
    outs = []
    for chunks in ([(0, V)], [(0, 384), (384, V)]):
        xt, tk = xt_cube.clone(), _tickets(R)
        grad, bg = torch.full((V, D), 7.0, device='cuda'), torch.full((D,), 7.0, device='cuda')
        for r0, r1 in chunks:
            L.call('cc_embed_grad_cs_reg', L.ptr(img), packed, r1 - r0, D, R, RP, L.ptr(xt[r0:]), L.ptr(grad[r0:]),
                   L.ptr(bg) if r1 == V else None, L.ptr(tk), *reg, r0, L.stream_ptr())
        torch.cuda.synchronize()
        assert int(xt.abs().sum().item()) == 0 and int(tk.abs().sum().item()) == 0
        outs.append((grad, bg))
    assert not bool((outs[0][0] == 7.0).any()) and not bool((outs[0][1] == 7.0).any())
    _same(outs[1], outs[0], ('grad', 'bias_grad'))
