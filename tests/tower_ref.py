"""Plain-numpy fp64 reference of the fused towers (csrc/tower.hip), one layer at a time, with the
per-element error bounds of tests/test_gpu_tower_elem.py and the layouts of every image the chains
write.  No GPU, no torch: tests/test_tower_ref_host.py holds this module to torch-CPU autograd.

Conventions (include/ccrec.h, cc_tower_args): chain layers i = 0..5 with K_i, N_i of chain_dims;
rows [0, B) use weights l = i, rows [B, R) use l = i + 3 for i >= 3.  A reference of one layer
takes that layer's inputs AS STORED (by the kernel under test, or by a simulated one), so exactly
one rounding step of the kernel separates it from the reference.

bf16 values travel as uint16 bit patterns (bits / from_bits) so every image comparison is bitwise.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff
UB = 2.0 ** -8          # the repo's conservative bf16 rounding step (half an ulp is 2^-9 relative)


def widths(d):
    return [d, 256, 128, 64, 128, 256, d]


def chain_dims(d):
    w = widths(d)
    return [(w[i], w[i + 1]) for i in range(6)]


def layer_of(i, reg):
    """Weight index l of chain layer i on the cube rows (reg = 0) or the regulariser rows (1)."""
    return i if i < 3 or not reg else i + 3


def branches(i, B, R):
    """(l, first row, end row) of every non-empty row range of chain layer i."""
    if i < 3:
        return [(i, 0, R)]
    return [(i, 0, B)] + ([(i + 3, B, R)] if R > B else [])


def layer_rows(l, B, R):
    """(chain layer, first row, end row) of weight index l: the rows its gradient sums over."""
    return (l, 0, R) if l < 3 else ((l, 0, B) if l < 6 else (l - 3, B, R))


# ------------------------------------------------------------------ bf16 (round to nearest even)
def bits(a):
    """fp32 -> bf16 bit patterns, round-to-nearest-even (csrc/common.hpp f2bf; finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def from_bits(b):
    """bf16 bit patterns -> fp64 values."""
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def round_bf16(a):
    return from_bits(bits(a))


def round_to(a, bf16):
    """fp64 -> the operand format's values (fp64 again)."""
    return round_bf16(a) if bf16 else np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------ inputs
Inputs = namedtuple('Inputs', 'd B R bf16 W b x0 gD3')


def make_inputs(d, B, R, bf16, seed):
    """Weights N(0, 2/K_i), biases N(0, 0.1^2), act[0] = relu(N(0, 1)), gD3 = N(0, 1), all rounded to
    the operand format (biases are fp32 in both).  Keeps every layer's share of positive
    pre-activations near one half (live_share), so every ReLU mask has both kinds of element."""
    rng = np.random.default_rng(seed)
    dims = chain_dims(d)
    W, b = [], []
    for l in range(9):
        K, N = dims[l if l < 6 else l - 3]
        W.append(round_to(rng.standard_normal((K, N)) * np.sqrt(2.0 / K), bf16))
        b.append((rng.standard_normal(N) * 0.1).astype(np.float32).astype(np.float64))
    x0 = round_to(np.maximum(rng.standard_normal((R, d)), 0.0), bf16)
    gD3 = round_to(rng.standard_normal((R, d)), bf16)
    return Inputs(d, B, R, bf16, W, b, x0, gD3)


def case_inputs(d, B, R, bf16):
    """The inputs every test of shape (d, B, R, bf16) uses (one seed per shape)."""
    return make_inputs(d, B, R, bf16, 1000 * d + 7 * R + B + int(bf16))


# (d, B, R, bf16) of every case of tests/test_gpu_tower_elem.py, by the kernel family it reaches
SHAPES = {
    'generic_f32': [(64, 32, 96, False), (256, 64, 64, False)],
    'generic_bf16': [(320, 32, 96, True), (512, 64, 64, True)],
    'fast': [(d, B, R, True) for d in (64, 128, 192, 256) for B, R in ((32, 96), (64, 64))],
    'wide': [(d, 32, 96, True) for d in (320, 384, 448, 512, 1024)],
    'dw': [(64, 32, 96, False), (256, 32, 96, True), (64, 64, 64, True), (128, 32, 160, True), (64, 32, 3104, True)],
}
ALL_SHAPES = sorted({s for v in SHAPES.values() for s in v})


# ------------------------------------------------------------------ one layer, fp64
def fwd_layer(inp, i, H):
    """relu(H W_l + b_l) of chain layer i from its stored input H [R][K_i]: (ref, eps).
    eps = (K_i + 4) 2^-24 (|H| |W_l| + |b_l|): fp32 accumulation in any order (bf16 products are
    exact in fp32; + 4: the fp32 operand path's product roundings and the bias add)."""
    K, N = chain_dims(inp.d)[i]
    ref, eps = np.zeros((inp.R, N)), np.zeros((inp.R, N))
    for l, lo, hi in branches(i, inp.B, inp.R):
        ref[lo:hi] = np.maximum(H[lo:hi] @ inp.W[l] + inp.b[l], 0.0)
        eps[lo:hi] = (K + 4) * U * (np.abs(H[lo:hi]) @ np.abs(inp.W[l]) + np.abs(inp.b[l]))
    return ref, eps


def bwd_layer(inp, i, G, H):
    """(G W_l^T) * (H > 0) of chain layer i from its stored output gradient G [R][N_i] and stored
    input H [R][K_i]: (ref, eps, mask).  eps = (N_i + 4) 2^-24 |G| |W_l^T| (zero where masked)."""
    K, N = chain_dims(inp.d)[i]
    ref, eps = np.zeros((inp.R, K)), np.zeros((inp.R, K))
    mask = H > 0
    for l, lo, hi in branches(i, inp.B, inp.R):
        ref[lo:hi] = (G[lo:hi] @ inp.W[l].T) * mask[lo:hi]
        eps[lo:hi] = (N + 4) * U * (np.abs(G[lo:hi]) @ np.abs(inp.W[l]).T) * mask[lo:hi]
    return ref, eps, mask


def stored_bound(ref, eps, bf16):
    """Bound on a value the kernel stores in the operand format: one bf16 rounding of the fp32
    value, or (fp32) the accumulation error alone."""
    return UB * (np.abs(ref) + eps) + eps if bf16 else eps


def dw_layer(inp, l, Hs, Gs):
    """gw_l = H^T G and gb_l = colsum G over the rows of weight index l, from the stored H_i / G_i
    (lists over the chain layers): (gw, gw_bound, gb, gb_bound); bounds (rows + 2) 2^-24 |H|^T |G|
    and (rows + 2) 2^-24 colsum |G| (fp32 operands: rows + 4, their products round)."""
    i, lo, hi = layer_rows(l, inp.B, inp.R)
    H, G = Hs[i][lo:hi], Gs[i][lo:hi]
    c = ((hi - lo) + (2 if inp.bf16 else 4)) * U
    return H.T @ G, c * (np.abs(H).T @ np.abs(G)), G.sum(0), c * np.abs(G).sum(0)


# ------------------------------------------------------------------ whole chains (the layers above, composed)
def chain_fwd(inp, rnd=lambda a: a):
    """act[0..6]; rnd is the storage rounding between layers (identity: exact fp64)."""
    acts = [inp.x0]
    for i in range(6):
        acts.append(rnd(fwd_layer(inp, i, acts[i])[0]))
    return acts


def chain_bwd(inp, acts, rnd=lambda a: a):
    """(G_0..G_5, gpre1): G_5 = gD3, G_{i-1} = rnd(layer i's dX), gpre1 = layer 0's dX (unrounded:
    the kernels keep it in fp32)."""
    Gs = [None] * 5 + [inp.gD3]
    for i in range(5, 0, -1):
        Gs[i - 1] = rnd(bwd_layer(inp, i, Gs[i], acts[i])[0])
    return Gs, bwd_layer(inp, 0, Gs[0], acts[0])[0]


def live_share(inp):
    """Per chain layer i = 0..5: the share of its output's elements with a positive pre-activation
    (exact fp64 chain), and the share of act[0] that is positive, first."""
    acts = chain_fwd(inp)
    return [float((a > 0).mean()) for a in acts]


# ------------------------------------------------------------------ layouts (any dtype; shapes only)
def ceil64(n):
    return (n + 63) // 64 * 64


def pack_rows(X):
    """act6p: X [R][W] as fragments (row block, j): [R/32][W/16][2][32][8], flat."""
    R, W = X.shape
    return np.ascontiguousarray(X.reshape(R // 32, 32, W // 16, 2, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


def unpack_rows(flat, R, W):
    return np.ascontiguousarray(flat.reshape(R // 32, W // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4)).reshape(R, W)


def pack_t(X, red=None, fill=0):
    """act6tp / hpt / gpt / gpre1p: X [R][W] transposed and packed, rows = the W features, reduction
    = batch rows padded to `red` with `fill`: [W/32][red/16][2][32][8], flat."""
    R, W = X.shape
    red = R if red is None else red
    Xp = np.full((red, W), fill, dtype=X.dtype)
    Xp[:R] = X
    return np.ascontiguousarray(Xp.reshape(red // 16, 2, 8, W // 32, 32).transpose(3, 0, 1, 4, 2)).reshape(-1)


def unpack_t(flat, W, red):
    """The inverse of pack_t: [red][W]."""
    return np.ascontiguousarray(flat.reshape(W // 32, red // 16, 2, 32, 8).transpose(1, 2, 4, 0, 3)).reshape(red, W)


def transpose_ld(X, ld=None, fill=0):
    """act6t (ld = R) / gpre1t (ld = ceil64(R)): X [R][W] as [W][ld], columns R.. = fill."""
    R, W = X.shape
    ld = R if ld is None else ld
    out = np.full((W, ld), fill, dtype=X.dtype)
    out[:, :R] = X.T
    return out


def ratio(err, bound):
    """max err / bound; where the bound is zero the error must be."""
    err, bound = np.asarray(err), np.asarray(bound)
    zero = bound == 0
    assert np.all(err[zero] == 0), 'an error where the bound is zero'
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0
