"""tests/tower_ref.py (the fp64 reference and bounds of tests/test_gpu_tower_elem.py) on the host:
the reference against torch-CPU autograd in float64 (so it is not its own judge), the layout helpers
against the index formulas of include/ccrec.h, the condition on the inputs (every ReLU mask has live
and dead elements), and the bounds themselves on a simulated kernel — the fp64 value rounded once,
which they must pass, and two single-fault mutations, which they must not."""
import numpy as np
import pytest
import torch

from tests import tower_ref as TR
from tests.gpu_helpers import rel_err


@pytest.mark.parametrize('d,B,R', [(64, 32, 96), (256, 64, 64), (320, 32, 96)])
def test_reference_matches_torch_autograd(d, B, R):
    inp = TR.case_inputs(d, B, R, True)
    acts = TR.chain_fwd(inp)
    Gs, gpre1 = TR.chain_bwd(inp, acts)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    W, b = [t(w) for w in inp.W], [t(x) for x in inp.b]
    pre0 = t(np.where(inp.x0 > 0, inp.x0, -1.0))     # act[0] = relu(pre0): gpre1 = dLoss / dpre0
    h, pres = torch.relu(pre0), [pre0]
    for i in range(6):
        parts = [h[lo:hi] @ W[l] + b[l] for l, lo, hi in TR.branches(i, B, R)]
        pre = torch.cat(parts, 0)
        pre.retain_grad()
        pres.append(pre)
        h = torch.relu(pre)
    # gD3 is dPre of d3 (include/ccrec.h): a loss that is linear in d3's pre-activation
    (pres[6] * torch.tensor(inp.gD3)).sum().backward()
    tol = 1e-12
    for i in range(7):
        assert rel_err(acts[i], torch.relu(pres[i]).detach().numpy()) < tol, i
    for i in range(6):         # G_i = dPre of chain layer i's output
        assert rel_err(Gs[i], pres[i + 1].grad.numpy()) < tol, i
    assert rel_err(gpre1, pre0.grad.numpy()) < tol
    for l in range(9 if R > B else 6):
        gw, _, gb, _ = TR.dw_layer(inp, l, acts, Gs)
        assert rel_err(gw, W[l].grad.numpy()) < tol, l
        assert rel_err(gb, b[l].grad.numpy()) < tol, l


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3, 0.0, 7.0], np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(TR.bits(x), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(TR.from_bits(TR.bits(x)), want.double().numpy())
    r = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(TR.bits(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_layout_helpers():
    R, W, FILL = 96, 64, 9999
    X = np.arange(R * W, dtype=np.int32).reshape(R, W)
    # act6p: fragment (row block t, j), lane l: row 32t + (l & 31), columns 16j + 8(l >> 5) .. + 8
    P = TR.pack_rows(X).reshape(R // 32, W // 16, 64, 8)
    for t, j, l in ((0, 0, 0), (2, 3, 37), (1, 2, 63), (2, 0, 31)):
        c = 16 * j + 8 * (l >> 5)
        assert np.array_equal(P[t, j, l], X[32 * t + (l & 31), c:c + 8])
    assert np.array_equal(TR.unpack_rows(TR.pack_rows(X), R, W), X)
    # act6tp / hpt / gpt: fragment (feature block t, j), lane l: feature 32t + (l & 31), batch rows
    # 16j + 8(l >> 5) .. + 8;  gpre1p: the same with the reduction padded to ceil64(R)
    for red in (R, TR.ceil64(R)):
        P = TR.pack_t(X, red, FILL).reshape(W // 32, red // 16, 64, 8)
        for t, j, l in ((0, 0, 0), (1, 5, 37), (1, 2, 63), (0, 3, 31)):
            r = 16 * j + 8 * (l >> 5)
            assert np.array_equal(P[t, j, l], X[r:r + 8, 32 * t + (l & 31)])
        assert np.all(P[:, R // 16:] == FILL)
        back = TR.unpack_t(TR.pack_t(X, red, FILL), W, red)
        assert np.array_equal(back[:R], X) and np.all(back[R:] == FILL)
    T = TR.transpose_ld(X, TR.ceil64(R), FILL)
    assert T.shape == (W, 128) and np.array_equal(T[:, :R], X.T) and np.all(T[:, R:] == FILL)
    assert np.array_equal(TR.transpose_ld(X), X.T)


@pytest.mark.parametrize('d,B,R,bf16', TR.ALL_SHAPES)
def test_inputs_keep_every_mask_mixed(d, B, R, bf16):
    """A mask test on rows that are all live, or all dead, checks nothing."""
    share = TR.live_share(TR.case_inputs(d, B, R, bf16))
    assert all(0.3 <= s <= 0.7 for s in share), share


def _simulate(inp):
    """A kernel that is right: every stored value is the fp64 value rounded once; dW / db are fp32
    sums (numpy's own order)."""
    rnd = lambda a: TR.round_to(a, inp.bf16)
    acts = TR.chain_fwd(inp, rnd)
    Gs, gpre1 = TR.chain_bwd(inp, acts, rnd)
    return acts, Gs, gpre1.astype(np.float32).astype(np.float64)


def _bwd_ratio(inp, i, got, Gs, acts, bf16):
    ref, eps, mask = TR.bwd_layer(inp, i, Gs[i], acts[i])
    if np.any(got[~mask] != 0):
        return np.inf
    return TR.ratio(np.abs(got - ref), TR.stored_bound(ref, eps, bf16) * mask)


@pytest.mark.parametrize('d,B,R,bf16', [(64, 32, 96, False), (256, 32, 96, True), (448, 32, 96, True),
                                        (64, 32, 3104, True)])
def test_bounds_pass_a_right_kernel_and_fail_a_wrong_one(d, B, R, bf16):
    inp = TR.case_inputs(d, B, R, bf16)
    acts, Gs, gpre1 = _simulate(inp)
    for i in range(6):
        ref, eps = TR.fwd_layer(inp, i, acts[i])
        assert TR.ratio(np.abs(acts[i + 1] - ref), TR.stored_bound(ref, eps, bf16)) <= 1, i
    for i in range(5, 0, -1):
        assert _bwd_ratio(inp, i, Gs[i - 1], Gs, acts, bf16) <= 1, i
    assert _bwd_ratio(inp, 0, gpre1, Gs, acts, False) <= 1
    f32 = lambda a: a.astype(np.float32)
    for l in range(9):
        i, lo, hi = TR.layer_rows(l, B, R)
        gw, bw, gb, bb = TR.dw_layer(inp, l, acts, Gs)
        H, G = acts[i][lo:hi], Gs[i][lo:hi]
        assert TR.ratio(np.abs(f32(H).T @ f32(G) - gw), bw) <= 1, l
        assert TR.ratio(np.abs(f32(G).sum(0, dtype=np.float32) - gb), bb) <= 1, l
        # one dropped 16-row step
        keep = np.r_[0:16, 32:hi - lo]
        assert TR.ratio(np.abs(H[keep].T @ G[keep] - gw), bw) > 1, l
        assert TR.ratio(np.abs(G[keep].sum(0) - gb), bb) > 1, l
    # one flipped mask element, either way, in every backward layer
    for i in range(5, -1, -1):
        got = (Gs[i - 1] if i else gpre1).copy()
        ref, _, mask = TR.bwd_layer(inp, i, Gs[i], acts[i])
        full = np.concatenate([Gs[i][lo:hi] @ inp.W[l].T for l, lo, hi in TR.branches(i, B, R)], 0)
        r, c = np.argwhere(~mask & (full != 0))[7]
        dead = got.copy()
        dead[r, c] = full[r, c]                       # a masked element left unmasked
        assert _bwd_ratio(inp, i, dead, Gs, acts, bf16 and i > 0) > 1, i
        live = np.argwhere(mask & (np.abs(ref) > np.median(np.abs(ref[mask]))))
        r, c = live[7]
        got[r, c] = 0.0                               # a live element masked off
        assert _bwd_ratio(inp, i, got, Gs, acts, bf16 and i > 0) > 1, i
